"""Markov diffusion of snapshots and edge lists on the device (ops.snapshot_markov, ops.markov_diffusion, rlap_markov.hip, DESIGN
4.23) against the host mirror (tests/csrc/markov_mirror.cc: rlap_amd/csrc/rlap_markov.h compiled with g++ -ffp-contract=off, the
rule run sparsely in the device's order), bit for bit: rows, values, offsets.  Keep decisions are then identical by construction;
the mirror itself is checked against the dense restatement in tests/test_markov_cpu.py.  Every call is made twice and must repeat
its bits.  This file: parameters and flags, ids without edges, inputs from the elimination, node_ptr batches of both diffusions,
and the adapters; tests/test_gpu_markov_regimes.py walks the regimes."""
import numpy as np
import pytest
import torch

import markov_mirror as mm
from util import ba_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mm.build(tmp_path_factory.mktemp("markov"))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def markov_twice(ops, sc, ptr, n, **kw):
    """(out, mptr, last_stats) of ops.snapshot_markov; the call is made twice and must give the same bits."""
    out, mptr = ops.snapshot_markov(sc, ptr, n, **kw)
    st = dict(ops.last_stats)
    out2, mptr2 = ops.snapshot_markov(sc, ptr, n, **kw)
    assert same_bits(out, out2) and torch.equal(mptr, mptr2), "the same call gave other bits"
    return out, mptr, st


def equals_mirror(lib, out, mptr, parts, normalize=False, **kw):
    """The device's (out, mptr) against the mirror run on every segment of `parts` (numpy rows): bit for bit."""
    mkw = dict(alpha=kw.get("alpha", 0.2), order=kw.get("order", 16), eps=kw.get("eps", 1e-4), weighted=kw.get("weighted", True),
               self_loop=kw.get("add_self_loop", True), zero_ok=kw.get("zero_ok", False))
    ptr = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])])
    want, wptr = mm.run_call(lib, np.concatenate(parts) if parts else np.empty((0, 3)), ptr, normalize=normalize, **mkw)
    assert mptr.tolist() == wptr.tolist(), "the offsets differ from the mirror's"
    assert same_bits(out.cpu(), torch.from_numpy(want)), "rows or values differ from the mirror's"


def graph_rows(n, seed, m=3):
    ei = np.asarray(ba_graph(n, m, seed))
    return mm.column_layout(ei, mm.symmetric_weights(ei, seed + 100))


@pytest.fixture(scope="module")
def ba300():
    return graph_rows(300, 21)


CASES = [dict(), dict(order=1), dict(order=2), dict(order=3), dict(alpha=0.0), dict(alpha=1.0), dict(alpha=0.0, order=3),
         dict(weighted=False), dict(add_self_loop=False), dict(add_self_loop=False, order=3, weighted=False),
         dict(normalize_out=True), dict(normalize_out=True, add_self_loop=False, order=2), dict(eps=1.2345e-3, order=5)]


@pytest.mark.parametrize("kw", CASES, ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "defaults")
def test_parameters_and_flags(ops, lib, ba300, kw):
    sc = torch.from_numpy(ba300).cuda()
    out, mptr, st = markov_twice(ops, sc, [0, sc.shape[0]], 300, **kw)
    assert st["order"] == kw.get("order", 16) and (st["small_tiles"], st["large_tiles"], st["groups"]) == (5, 0, 1)
    assert st["host_syncs"] == 3 and st["launches"] == 2 + 4 and st["rows_needed"] == out.shape[0] == int(mptr[-1])
    equals_mirror(lib, out, mptr, [ba300], normalize=kw.get("normalize_out", False), **kw)
    i, j, v = out[:, 0].long(), out[:, 1].long(), out[:, 2]
    kf, of = torch.sort(i * 300 + j)
    kb, ob = torch.sort(j * 300 + i)
    assert torch.equal(kf, kb) and same_bits(v[of], v[ob])                       # exactly symmetric
    assert bool((kf[1:] > kf[:-1]).all()) and torch.equal(of, torch.arange(of.numel(), device=of.device))   # ascending (i, j)


def test_ids_without_edges(ops, lib):
    """Ids 0 and 201 have no edges: no row without the self loop, the one entry alpha + (1/D) sum_k beta^k with it."""
    ei = np.asarray(ba_graph(200, 3, 4)) + 1
    w = mm.symmetric_weights(ei, 3)
    n = 202
    sc = mm.column_layout(ei, w)
    rows = np.concatenate([[[0.0, 0.0, 0.0]], sc, [[201.0, 201.0, 0.0]]])
    t, tw = torch.from_numpy(ei).cuda(), torch.from_numpy(w).cuda()
    for loop in (False, True):
        for normalize in (False, True):
            gi, gw = ops.markov_diffusion(t, tw, n, order=5, add_self_loop=loop, normalize_out=normalize)
            gi2, gw2 = ops.markov_diffusion(t, tw, n, order=5, add_self_loop=loop, normalize_out=normalize)
            assert torch.equal(gi, gi2) and same_bits(gw, gw2)
            raw, norm = mm.run(lib, rows, order=5, self_loop=loop, zero_ok=True)
            want = norm if normalize else raw
            assert torch.equal(gi.cpu(), torch.from_numpy(want[:, :2].astype(np.int64).T.copy()))
            assert same_bits(gw.cpu(), torch.from_numpy(want[:, 2].copy()))
            for v in (0, n - 1):
                row = gi[0] == v
                if not loop:
                    assert int(row.sum()) == 0 and int((gi[1] == v).sum()) == 0
                else:
                    assert gi[1][row].tolist() == [v]
                    if not normalize:
                        assert float(gw[row][0]) == pytest.approx(0.2 + sum(0.8 ** k for k in range(6)) / 5, rel=1e-14)


def test_snapshots_of_a_depths_call_with_node_ptr(ops, lib):
    """The (sc, ptr) of a views=2 depths call on a batch of three graphs: every segment equals the call on it alone and the mirror."""
    sizes = [40, 150, 70]
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    eis = [np.asarray(ba_graph(k, 3, 5 + k)) + int(o) for k, o in zip(sizes, node_ptr[:-1])]
    ei = torch.from_numpy(np.concatenate(eis, 1))
    n = int(node_ptr[-1])
    nr = [[[k // 4 for k in sizes]] * 2, [[k // 2 for k in sizes]] * 2]         # (D, K, G)
    sc, ptr = ops.approximate_cholesky_depths(ei.cuda(), None, n, nr, "degree", "asc", node_ptr=node_ptr.tolist(), views=2, seed=3,
                                              return_device="same")
    S = ptr.numel() - 1
    assert S == 2 * 2 * 3
    out, mptr, st = markov_twice(ops, sc, ptr, n, node_ptr=node_ptr.tolist(), order=4, eps=1e-3)
    assert st["small_tiles"] == sum(-(-int(k) // 64) for k in
                                                      [len(torch.unique(sc[int(ptr[s]):int(ptr[s + 1]), :2])) for s in range(S)])
    pp, mp = ptr.tolist(), mptr.tolist()
    host = sc.cpu().numpy()
    equals_mirror(lib, out, mptr, [host[pp[s]:pp[s + 1]] for s in range(S)], order=4, eps=1e-3)
    for s in range(S):
        g = s % 3
        alone, ap, _ = markov_twice(ops, sc[pp[s]:pp[s + 1]], [0, pp[s + 1] - pp[s]], n, order=4, eps=1e-3)
        assert same_bits(out[mp[s]:mp[s + 1]], alone), s
        ids = alone[:, :2]
        assert ids.numel() == 0 or (int(ids.min()) >= node_ptr[g] and int(ids.max()) < node_ptr[g + 1])


def batch(sizes, seed):
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    eis, ws = [], []
    for g, k in enumerate(sizes):
        e = np.asarray(ba_graph(k, 2, seed + g)) if k > 3 else np.array([[0, 1], [1, 0]])[:, :2 * (k > 1)]
        eis.append(e + int(node_ptr[g]))
        ws.append(mm.symmetric_weights(e, seed + g) if e.size else np.zeros(0))
    return np.concatenate(eis, 1), np.concatenate(ws), node_ptr


@pytest.mark.parametrize("which", ["markov", "ppr"])
def test_diffusions_of_a_batch_with_node_ptr(ops, which):
    """markov_diffusion and ppr_diffusion with node_ptr against one call per graph, bit for bit (graph 2 is one id without edges)."""
    sizes = [33, 2, 1, 130, 64]
    ei, w, node_ptr = batch(sizes, 11)
    perm = np.random.RandomState(0).permutation(ei.shape[1])                     # rows in no particular order
    t, tw = torch.from_numpy(ei[:, perm]).cuda(), torch.from_numpy(w[perm]).cuda()
    fn = ops.markov_diffusion if which == "markov" else ops.ppr_diffusion
    kw = dict(order=6, eps=1e-3) if which == "markov" else dict(eps=1e-3, add_self_loop=True)
    gi, gw = fn(t, tw, int(node_ptr[-1]), node_ptr=node_ptr.tolist(), **kw)
    st = dict(ops.last_stats)
    gi2, gw2 = fn(t, tw, int(node_ptr[-1]), node_ptr=node_ptr.tolist(), **kw)
    assert torch.equal(gi, gi2) and same_bits(gw, gw2)
    if which == "markov":
        assert (st["small_tiles"], st["large_tiles"]) == (1 + 1 + 1 + 3 + 1, 0)
    parts_i, parts_w = [], []
    for g, k in enumerate(sizes):
        lo, hi = int(node_ptr[g]), int(node_ptr[g + 1])
        sel = (t[0] >= lo) & (t[0] < hi)
        ai, aw = fn(t[:, sel] - lo, tw[sel], k, **kw)
        parts_i.append(ai + lo)
        parts_w.append(aw)
    assert torch.equal(gi, torch.cat(parts_i, 1)) and same_bits(gw, torch.cat(parts_w))
    whole_i, _ = fn(t, tw, int(node_ptr[-1]), **kw)                              # one segment: the same graphs, (sum n_g)^2 of work
    assert whole_i.shape[1] == gi.shape[1] or which == "ppr"
    bad = torch.cat([t, torch.tensor([[0, 40], [40, 0]], device=t.device)], 1)
    with pytest.raises(ValueError, match="joins two graphs"):
        fn(bad, torch.cat([tw, torch.ones(2, dtype=tw.dtype, device=tw.device)]), int(node_ptr[-1]), node_ptr=node_ptr.tolist(), **kw)


def test_ppr_diffusion_without_node_ptr_is_the_snapshot_call(ops):
    """The default keeps its bits: ppr_diffusion(ei, w, n) is snapshot_ppr on the rows grouped by column."""
    ei = np.asarray(ba_graph(150, 3, 2))
    w = mm.symmetric_weights(ei, 6)
    gi, gw = ops.ppr_diffusion(torch.from_numpy(ei).cuda(), torch.from_numpy(w).cuda(), 150)
    sc = torch.from_numpy(mm.column_layout(ei, w)).cuda()
    out, pptr = ops.snapshot_ppr(sc, [0, sc.shape[0]], 150)
    assert torch.equal(gi, out[:, :2].long().t()) and same_bits(gw, out[:, 2].contiguous()) and pptr.tolist() == [0, out.shape[0]]


def test_markov_diffusion_against_the_dense_adapter(ops):
    """The device against adapters.compute_markov_diffusion on the same device and tensors: the pattern, and values to the bound
    of tests/test_markov_cpu.py (the gap to eps asserted first)."""
    from rlap_amd.adapters import compute_markov_diffusion
    n, D, eps = 257, 16, 1.2345e-3
    ei = np.asarray(ba_graph(n, 3, 9))
    w = mm.symmetric_weights(ei, 2)
    t, tw = torch.from_numpy(ei).cuda(), torch.from_numpy(w).cuda()
    _, M = mm.dense(mm.column_layout(ei, w), 0.2, D)
    assert not np.any(np.abs(M - eps) <= 1e-9 * eps)
    gi, gw = ops.markov_diffusion(t, tw, n, order=D, eps=eps)
    ri, rw = compute_markov_diffusion(t, tw, n, alpha=0.2, degree=D, sp_eps=eps)
    assert torch.equal(gi, ri)
    rel = float(((gw - rw).abs() / rw).max())
    print(f"device against the dense adapter: max rel diff {rel:.3g}")
    assert rel <= 2 * (D + 2) * (n + 4) * 2.0 ** -53


def test_depths_adapter_diffuse_kind_markov(ops):
    """rLapDepths.diffuse(kind="markov") and diffuse_plan feeding SnapshotGCNConv once: shape, and forward equals the propagation
    of the same rows through edge_list_plan."""
    from rlap_amd import adapters
    n = 120
    ei = torch.from_numpy(np.asarray(ba_graph(n, 3, 1))).cuda()
    x = torch.randn(n, 8, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).cuda()
    d = adapters.rLapDepths(fracs=(0.2, 0.5), o_v="degree", o_n="asc", keep_weights=True, seed=1, views=2)
    g = adapters.Graph(x, ei, None)
    graphs = d.diffuse(g, kind="markov", order=4, eps=1e-3)
    assert ops.last_stats["order"] == 4 and len(graphs) == 2 and len(graphs[0]) == 2
    _, sc, ptr, num_nodes = d._snapshots(g)
    out, mptr = ops.snapshot_markov(sc, ptr, num_nodes, order=4, eps=1e-3)
    mp = mptr.tolist()
    for r in range(2):
        for k in range(2):
            part = out[mp[k * 2 + r]:mp[k * 2 + r + 1]]
            assert torch.equal(graphs[r][k].edge_index, part[:, :2].long().t()) and same_bits(graphs[r][k].edge_weights, part[:, 2].contiguous())
    plan = d.diffuse_plan(g, kind="markov", order=4, eps=1e-3)
    conv = adapters.SnapshotGCNConv(8, 5).to(device=x.device, dtype=torch.float64)
    y = conv(x, plan)
    assert tuple(y.shape) == (4, n, 5)
    ref = ops.edge_list_plan(out, mptr, n, weighted=True, add_self_loops=True, fill_value=1.0, normalize=True, directions="both")
    assert same_bits(y.detach(), conv(x, ref).detach())
