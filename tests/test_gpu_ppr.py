"""PPR diffusion of snapshots on the device (ops.snapshot_ppr, ops.ppr_diffusion, rlap_snapshot_ppr): against float64 numpy inverses
and the dense adapter on small snapshots, bit-exact batching and repeatability, edge cases and layout errors, and a BA(50k, 5)
snapshot against an independent CG solve in torch."""
import numpy as np
import pytest
import torch

from ppr_dense import dense_ppr, to_dense
from util import ba_graph, grid2d, path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def check_segment(ops, part, out, tol, eps=1e-4, **kw):
    nodes, S0, S = dense_ppr(part, eps=eps, **kw)
    assert not np.any(np.abs(S0 - eps) <= 2 * tol), "an exact entry lies within 2 tol of eps: the keep decision is not determined"
    got, keep = to_dense(out, nodes)
    assert np.array_equal(keep, S0 >= eps)
    assert np.allclose(got, S, rtol=1e-7, atol=1e-12)
    # row-major order, ascending i then j
    key = out[:, 0].long() * (int(nodes.max()) + 1) + out[:, 1].long()
    assert bool((key[1:] > key[:-1]).all())


def sc_of(ei, w=None):
    """A symmetric edge list as op-style rows [row, col, w], every column's rows contiguous."""
    ei = torch.as_tensor(np.ascontiguousarray(ei))
    o = torch.argsort(ei[1] * (int(ei.max()) + 1) + ei[0])
    w = torch.ones(ei.shape[1], dtype=torch.float64) if w is None else torch.as_tensor(w, dtype=torch.float64)
    return torch.stack([ei[0][o].double(), ei[1][o].double(), w[o]], 1).cuda()


@pytest.fixture(scope="module")
def ba300(ops):
    n = 300
    ei = torch.from_numpy(ba_graph(n, 4, 21)).cuda()
    return n, ei, {o_v: ops.approximate_cholesky(ei, None, n, n // 2, o_v, "asc", seed=5, return_device="same")
                   for o_v in ("random", "degree", "coarsen")}


@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_single_snapshot(ops, ba300, o_v):
    n, _, scs = ba300
    sc = scs[o_v]
    out, pptr = ops.snapshot_ppr(sc, [0, sc.shape[0]], n, tol=1e-12)
    assert pptr.tolist() == [0, out.shape[0]]
    assert ops.last_stats["steps"] == 41 and ops.last_stats["small_tiles"] > 0
    check_segment(ops, sc, out, 1e-12)


@pytest.mark.parametrize("kw", [{"weighted": False}, {"self_loop": True}, {"normalize": False}])
def test_single_snapshot_options(ops, ba300, kw):
    n, _, scs = ba300
    sc = scs["degree"]
    names = {"weighted": "weighted", "self_loop": "add_self_loop", "normalize": "normalize_out"}
    out, _ = ops.snapshot_ppr(sc, [0, sc.shape[0]], n, tol=1e-12, **{names[k]: v for k, v in kw.items()})
    check_segment(ops, sc, out, 1e-12, **kw)


def test_same_rows_as_dense_adapter(ops, ba300):
    from rlap_amd.adapters import compute_ppr
    n, _, scs = ba300
    sc = scs["random"]
    ei = sc[:, :2].long().t()
    nodes = torch.unique(ei, sorted=True)
    relabel = torch.full((n,), -1, dtype=torch.int64, device=ei.device)
    relabel[nodes] = torch.arange(nodes.numel(), device=ei.device)
    d_ei, d_w = compute_ppr(relabel[ei], sc[:, 2], nodes.numel())
    out, _ = ops.snapshot_ppr(sc, [0, sc.shape[0]], n)
    assert torch.equal(out[:, :2].long().t(), nodes[d_ei])
    assert torch.allclose(out[:, 2], d_w, rtol=1e-7, atol=1e-12)


def segments_equal_alone(ops, sc, ptr, n, **kw):
    out, pptr = ops.snapshot_ppr(sc, ptr, n, **kw)
    out2, pptr2 = ops.snapshot_ppr(sc, ptr, n, **kw)
    assert torch.equal(out, out2) and torch.equal(pptr, pptr2)
    p = torch.as_tensor(ptr).tolist()
    pp = pptr.tolist()
    for s in range(len(p) - 1):
        alone, ap = ops.snapshot_ppr(sc[p[s]:p[s + 1]], [0, p[s + 1] - p[s]], n)
        assert torch.equal(out[pp[s]:pp[s + 1]], alone), s
        assert ap.tolist() == [0, pp[s + 1] - pp[s]]
    return out, pptr


def test_batches_bit_exact(ops):
    n = 600
    ei = torch.from_numpy(ba_graph(n, 4, 2)).cuda()
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, [n // 4, n // 2], "degree", "asc", views=2, seed=1, return_device="same")
    out, pptr = segments_equal_alone(ops, sc, ptr.tolist(), n)
    assert pptr.numel() == 5
    # a node_ptr batch of three graphs, with depths
    gs = [ba_graph(200, 3, 1), grid2d(10, 12), ba_graph(5000, 4, 3)]
    ns = [200, 120, 5000]
    off = np.concatenate([[0], np.cumsum(ns)])
    big = torch.from_numpy(np.concatenate([g + off[i] for i, g in enumerate(gs)], 1)).cuda()
    N = int(off[-1])
    sc, ptr = ops.approximate_cholesky_depths(big, None, N, [40, 80], "degree", "asc", node_ptr=off.tolist(), return_device="same")
    out, pptr = ops.snapshot_ppr(sc, ptr, N, node_ptr=off.tolist())
    assert ops.last_stats["large_tiles"] > 0 and ops.last_stats["small_tiles"] > 0   # both regimes in one call
    out_flat, pptr_flat = segments_equal_alone(ops, sc, ptr.tolist(), N)
    assert torch.equal(out, out_flat) and torch.equal(pptr, pptr_flat)


@pytest.mark.parametrize("name", ["path", "grid"])
def test_path_and_grid(ops, name):
    ei = path(50) if name == "path" else grid2d(9, 11)
    sc = sc_of(ei)
    n = int(ei.max()) + 1
    for self_loop in (False, True):
        out, _ = ops.snapshot_ppr(sc, [0, sc.shape[0]], n, tol=1e-12, add_self_loop=self_loop)
        check_segment(ops, sc, out, 1e-12, self_loop=self_loop)


def test_empty_small_and_vanishing(ops):
    two = sc_of(np.array([[0, 1], [1, 0]]), [2.0, 2.0])
    grid = sc_of(grid2d(5, 6))
    sc = torch.cat([two, grid])
    m2 = two.shape[0]
    ptr = [0, 0, m2, m2, sc.shape[0], sc.shape[0]]
    out, pptr = ops.snapshot_ppr(sc, ptr, 30)
    pp = pptr.tolist()
    assert pp[0] == pp[1] == 0 and pp[2] == pp[3] and pp[4] == pp[5] == out.shape[0]
    check_segment(ops, two, out[pp[1]:pp[2]], 1e-10)
    check_segment(ops, grid, out[pp[3]:pp[4]], 1e-10)
    # eps above every entry: every row vanishes
    out, pptr = ops.snapshot_ppr(sc, ptr, 30, eps=0.99)
    assert out.shape[0] == 0 and pptr.tolist() == [0] * 6
    # no rows at all
    out, pptr = ops.snapshot_ppr(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), [0, 0, 0], 5)
    assert out.shape[0] == 0 and pptr.tolist() == [0, 0, 0]


def test_layout_errors_and_inputs_unchanged(ops):
    sc = sc_of(grid2d(4, 5))
    before = sc.clone()
    ptr = torch.tensor([0, sc.shape[0]], dtype=torch.int64, device="cuda")
    pb = ptr.clone()
    ops.snapshot_ppr(sc, ptr, 20)
    assert torch.equal(sc, before) and torch.equal(ptr, pb)
    bad = sc.clone()
    bad[[0, -1]] = bad[[-1, 0]]                            # column 0 split into two blocks
    with pytest.raises(ValueError):
        ops.snapshot_ppr(bad, [0, bad.shape[0]], 20)
    nocol = torch.cat([sc, torch.tensor([[25.0, 0.0, 1.0]], dtype=torch.float64, device="cuda")])
    nocol = nocol[torch.argsort(nocol[:, 1], stable=True)]
    with pytest.raises(ValueError):                        # row id 25 without a column of its own
        ops.snapshot_ppr(nocol, [0, nocol.shape[0]], 30)
    neg = sc.clone()
    neg[3, 2] = -1.0
    with pytest.raises(ValueError):                        # a weight <= 0, found on the device
        ops.snapshot_ppr(neg, [0, neg.shape[0]], 20)
    assert torch.equal(sc, before)


def cg_columns(sc, nodes, src, alpha, tol=1e-14, iters=500):
    """x_j of M x = alpha e_j for the sources `src` (local indices) by conjugate gradients in float64 torch."""
    k = nodes.numel()
    pos = torch.full((int(nodes.max()) + 1,), -1, dtype=torch.int64, device=sc.device)
    pos[nodes] = torch.arange(k, device=sc.device)
    r_, c_, w = pos[sc[:, 0].long()], pos[sc[:, 1].long()], sc[:, 2]
    d = torch.zeros(k, dtype=torch.float64, device=sc.device).index_add_(0, r_, w)
    a = (1 - alpha) * w / torch.sqrt(d[r_] * d[c_])

    def mv(X):
        Y = X.clone()
        Y.index_add_(0, r_, -a[:, None] * X[c_])
        return Y
    B = torch.zeros((k, src.numel()), dtype=torch.float64, device=sc.device)
    B[src, torch.arange(src.numel(), device=sc.device)] = alpha
    X = torch.zeros_like(B)
    R = B.clone()
    P = R.clone()
    rr = (R * R).sum(0)
    for _ in range(iters):
        Q = mv(P)
        st = rr / (P * Q).sum(0)
        X += st * P
        R -= st * Q
        rn = (R * R).sum(0)
        if float(rn.max().sqrt()) < tol:
            break
        P = R + (rn / rr) * P
        rr = rn
    return X


def test_large_segment(ops):
    n = 50_000
    from rlap_amd import graphs
    ei = graphs.barabasi_albert(n, 5, 11).cuda()
    sc = ops.approximate_cholesky(ei, None, n, n // 2, "degree", "asc", seed=1, return_device="same")
    m = sc.shape[0]
    out, _ = ops.snapshot_ppr(sc, [0, m], n)
    st = dict(ops.last_stats)
    assert st["large_tiles"] > 0 and st["small_tiles"] == 0
    i, j, v = out[:, 0].long(), out[:, 1].long(), out[:, 2]
    kf, of = torch.sort(i * n + j)
    kb, ob = torch.sort(j * n + i)
    assert torch.equal(kf, kb) and torch.equal(v[of], v[ob])       # exactly symmetric
    assert bool((v > 0).all())
    nodes = torch.unique(sc[:, :2].long())
    diag = i[i == j]
    assert torch.equal(torch.sort(diag)[0], nodes)
    raw, _ = ops.snapshot_ppr(sc, [0, m], n, normalize_out=False)
    g = torch.Generator().manual_seed(0)
    src = torch.randperm(nodes.numel(), generator=g)[:64].cuda()
    X = cg_columns(sc, nodes, src, 0.2)
    ri, rj, rv = raw[:, 0].long(), raw[:, 1].long(), raw[:, 2]
    pos = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    pos[nodes] = torch.arange(nodes.numel(), device="cuda")
    col = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    col[nodes[src]] = torch.arange(64, device="cuda")
    sel = col[rj] >= 0
    ref = X[pos[ri[sel]], col[rj[sel]]]
    assert float((rv[sel] - ref).abs().max()) <= 1e-9
    kept = torch.zeros_like(X, dtype=torch.bool)
    kept[pos[ri[sel]], col[rj[sel]]] = True
    assert bool(kept[X >= 1e-4 + 1e-9].all())


def test_ppr_diffusion_plain_graph(ops):
    from rlap_amd.adapters import compute_ppr
    n0 = 200
    ei = ba_graph(n0, 3, 4)
    n = n0 + 2                                   # two ids without edges
    rs = np.random.RandomState(1)
    dup = ei[:, rs.choice(ei.shape[1], 30, replace=False)]
    dup = np.concatenate([dup, dup[::-1]], 1)    # duplicates in both directions keep the adjacency symmetric
    allei = np.concatenate([ei, dup], 1)
    allei = allei[:, rs.permutation(allei.shape[1])]
    t = torch.from_numpy(np.ascontiguousarray(allei)).cuda()
    gi, gw = ops.ppr_diffusion(t, None, n, add_self_loop=True)
    ri, rw = compute_ppr(t, None, n, add_self_loop=True)
    assert torch.equal(gi, ri)
    assert torch.allclose(gw, rw, rtol=1e-7, atol=1e-12)
    w = torch.rand(allei.shape[1], dtype=torch.float64, device="cuda")   # asymmetric weights, then an asymmetric pattern
    with pytest.raises(ValueError, match="not symmetric"):
        ops.ppr_diffusion(t, w, n)
    with pytest.raises(ValueError, match="not symmetric"):
        ops.ppr_diffusion(t[:, 1:], None, n)


def test_depths_diffuse_layout(ops):
    from rlap_amd.adapters import rLapDepths
    n = 800
    ei = torch.from_numpy(ba_graph(n, 4, 6)).cuda()
    x = torch.randn(n, 3, device="cuda")
    for views in (None, 2):
        aug = rLapDepths((0.1, 0.3, 0.5), o_v="degree", seed=3, views=views)
        gs = aug.diffuse((x, ei, None))
        _, sc, ptr, nn = aug._snapshots((x, ei, None))
        out, pptr = ops.snapshot_ppr(sc, ptr, nn)
        pp = pptr.tolist()
        R = 1 if views is None else views
        flat = gs if views is None else [gs[r][k] for k in range(3) for r in range(R)]
        assert len(flat) == 3 * R
        for s, g in enumerate(flat):
            assert g.x is x
            assert torch.equal(g.edge_index, out[pp[s]:pp[s + 1], :2].long().t())
            assert torch.equal(g.edge_weights, out[pp[s]:pp[s + 1], 2])
