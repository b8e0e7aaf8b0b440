"""Encoder-ready snapshots on the device (ops.snapshot_gcn_norm, rlap_snapshot_gcn_norm) and the adapters' gcn_norm keyword.

The yardstick of every result is the torch formulation below (PyG's gcn_norm restated; PyG itself is not installed), written once and
independent of the code under test, per segment, in float64 on the CPU: mask row != col, loop weights by assignment in input order,
cat with arange(lo, hi), deg = zeros(n).index_add_(0, dst, w), dis = deg.pow(-0.5) with inf -> 0, dis[src] * w * dis[dst].

Integers are compared with torch.equal.  float64 values: relative error at most (16 + 2 L) * 2^-53, L the longest column block of the
call plus one -- a sum of L positive terms has relative error below (L - 1) u in any order (u = 2^-53), the yardstick's order and the
device's differ, a degree enters an entry twice under a square root (half the error each), and the remaining operations (a square
root, a reciprocal or pow, two products, on both sides) are bounded by 16 roundings.  Unweighted degrees are exact integers: 16 u.
float32 values equal the float64 result of the same call rounded once, and lie within 2^-23 relative of the yardstick's .float()."""
import numpy as np
import pytest
import torch

from util import ba_graph

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
HOST_SYNCS = 1          # the error words and the loop-row count, read back together


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def torch_segment(part, lo, hi, weighted, add_self_loops=True, fill=1.0, normalize=True):
    """(src, dst, val) of one segment with id range [lo, hi): the torch formulation, float64 on the CPU."""
    part = part.detach().cpu().double()
    src, dst = part[:, 0].long(), part[:, 1].long()
    w = part[:, 2].clone() if weighted else torch.ones(part.shape[0], dtype=torch.float64)
    if add_self_loops:
        mask = src != dst
        loop_w = torch.full((hi - lo,), float(fill), dtype=torch.float64)
        for i, wi in zip(src[~mask].tolist(), w[~mask].tolist()):      # by assignment in input order: the last loop row wins
            loop_w[i - lo] = wi
        ar = torch.arange(lo, hi, dtype=torch.int64)
        src, dst, w = torch.cat([src[mask], ar]), torch.cat([dst[mask], ar]), torch.cat([w[mask], loop_w])
    if not normalize:
        return src, dst, w
    deg = torch.zeros(max(hi, 1), dtype=torch.float64).index_add_(0, dst, w)
    dis = deg.pow(-0.5)
    dis[dis == float("inf")] = 0.0
    return src, dst, dis[src] * w * dis[dst]


def torch_formulation(sc, ptr, num_nodes, node_ptr=None, **kw):
    """(edge_index, val, eptr) of a whole call, on the CPU."""
    p = torch.as_tensor(ptr).tolist()
    G = len(node_ptr) - 1 if node_ptr is not None else 1
    srcs, dsts, vals, e = [], [], [], [0]
    for s in range(len(p) - 1):
        lo, hi = (node_ptr[s % G], node_ptr[s % G + 1]) if node_ptr is not None else (0, num_nodes)
        a, b, v = torch_segment(sc[p[s]:p[s + 1]], int(lo), int(hi), **kw)
        srcs.append(a), dsts.append(b), vals.append(v)
        e.append(e[-1] + a.numel())
    ei = torch.stack([torch.cat(srcs), torch.cat(dsts)])
    return ei, torch.cat(vals), torch.tensor(e, dtype=torch.int64)


def longest_block(sc, ptr):
    """The longest run of one column id inside a segment (0 for no rows)."""
    p = torch.as_tensor(ptr).tolist()
    best = 0
    for s in range(len(p) - 1):
        col = sc[p[s]:p[s + 1], 1]
        if col.numel():
            best = max(best, int(torch.unique_consecutive(col, return_counts=True)[1].max()))
    return best


def assert_values(got, ref, bound, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, f"{what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    if ref.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()), f"{what}: a value is not finite"
    rel = ((got - ref).abs() / ref.abs().clamp_min(1e-300)).max().item()
    exact_zero = bool(((ref == 0) == (got == 0)).all())
    print(f"{what}: max relative error {rel:.3e} (bound {bound:.3e})")
    assert exact_zero and rel <= bound, f"{what}: relative error {rel:.3e} above {bound:.3e}"


def check_call(ops, sc, ptr, n, what, node_ptr=None, **kw):
    """One configuration against the yardstick in float64 and float32; returns the float64 result."""
    weighted = kw.get("weighted", False)
    ykw = {"weighted": weighted, "add_self_loops": kw.get("add_self_loops", True), "fill": kw.get("fill_value", 1.0),
           "normalize": kw.get("normalize", True)}
    r_ei, r_val, r_eptr = torch_formulation(sc, ptr, n, node_ptr=node_ptr, **ykw)
    L = longest_block(sc, ptr) + 1
    bound = (16 + 2 * L) * U if weighted else 16 * U
    ei, val, eptr = ops.snapshot_gcn_norm(sc, ptr, n, node_ptr=node_ptr, dtype=torch.float64, **kw)
    assert ops.last_stats["host_syncs"] == HOST_SYNCS
    assert ei.dtype == torch.int64 and ei.is_contiguous() and ei.is_cuda and val.dtype == torch.float64 and eptr.dtype == torch.int64
    assert ei.shape == r_ei.shape, f"{what}: {tuple(ei.shape)} vs {tuple(r_ei.shape)}"
    assert torch.equal(ei.cpu(), r_ei), f"{what}: edge_index differs"
    assert torch.equal(eptr.cpu(), r_eptr), f"{what}: eptr differs"
    assert ops.last_stats["entries"] == r_ei.shape[1]
    assert_values(val, r_val, bound, f"{what} f64")
    ei32, val32, eptr32 = ops.snapshot_gcn_norm(sc, ptr, n, node_ptr=node_ptr, dtype=torch.float32, **kw)
    assert val32.dtype == torch.float32 and torch.equal(ei32, ei) and torch.equal(eptr32, eptr)
    assert torch.equal(val32.view(torch.int32), val.float().view(torch.int32)), f"{what}: float32 is not the float64 value rounded once"
    assert_values(val32, r_val.float(), 2.0 ** -23, f"{what} f32")
    # the same call twice
    ei2, val2, eptr2 = ops.snapshot_gcn_norm(sc, ptr, n, node_ptr=node_ptr, dtype=torch.float64, **kw)
    assert torch.equal(ei2, ei) and torch.equal(val2.view(torch.int64), val.view(torch.int64)) and torch.equal(eptr2, eptr)
    return ei, val, eptr


def depths_views(ops, n, m, seed, o_v, ts, views=2, node_ptr=None):
    ei = torch.from_numpy(ba_graph(n, m, seed)).cuda()
    return ops.approximate_cholesky_depths(ei, None, n, ts, o_v, "asc", views=views, node_ptr=node_ptr, seed=11, return_device="same")


def batch_snapshots(ops, sizes, views=2):
    """Depths x views of a batch of BA graphs of the given sizes (a graph of one vertex has no edge)."""
    node_ptr = [0] + [int(v) for v in np.cumsum(sizes)]
    parts = [ba_graph(k, 3, 40 + g) + node_ptr[g] for g, k in enumerate(sizes) if k >= 4]
    ei = torch.from_numpy(np.concatenate(parts, 1)).cuda()
    n = node_ptr[-1]
    ts = torch.tensor([[[k // 4 for k in sizes]] * views, [[k // 2 for k in sizes]] * views])
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, ts, "random", "asc", node_ptr=node_ptr, views=views, seed=4, return_device="same")
    assert ptr.numel() == 2 * views * len(sizes) + 1
    return n, sc, ptr, node_ptr


# ------------------------------------------------------------------------------------------------ 1. depths x views results
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_depths_views(ops, o_v, weighted):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, o_v, [n // 8, n // 4, n // 2])
    assert ptr.numel() == 7 and not bool((sc[:, 0] == sc[:, 1]).any())
    ei, val, eptr = check_call(ops, sc, ptr, n, f"{o_v} weighted={weighted}", weighted=weighted)
    # an elimination result has no loop rows: every slot of the allocation is written and nothing is copied
    m, S = sc.shape[0], 6
    assert ops.last_stats["entries"] == m + S * n and ops.last_stats["loops_removed"] == 0
    assert ei.untyped_storage().data_ptr() == ei.data_ptr() and ei.untyped_storage().nbytes() == 2 * (m + S * n) * 8
    # a views x depths call equals the concatenation of per-segment calls bit for bit
    p = ptr.tolist()
    parts = [ops.snapshot_gcn_norm(sc[p[s]:p[s + 1]], [0, p[s + 1] - p[s]], n, weighted=weighted, dtype=torch.float64) for s in range(S)]
    assert torch.equal(torch.cat([q[0] for q in parts], 1), ei)
    assert torch.equal(torch.cat([q[1] for q in parts]).view(torch.int64), val.view(torch.int64))
    # eliminated ids: their loop has value exactly 1
    e = eptr.tolist()
    for s in range(S):
        present = torch.zeros(n, dtype=torch.bool, device="cuda")
        present[sc[p[s]:p[s + 1], :2].long().reshape(-1)] = True
        loops = val[e[s + 1] - n:e[s + 1]]
        assert bool((~present).any()) and bool((loops[~present] == 1.0).all())
        assert torch.equal(ei[0, e[s + 1] - n:e[s + 1]], torch.arange(n, device="cuda"))


def test_conversion_alone_is_bit_exact(ops):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    ei, w, eptr = ops.snapshot_gcn_norm(sc, ptr, n, weighted=True, add_self_loops=False, normalize=False, dtype=torch.float64)
    assert ei.is_contiguous() and ei.dtype == torch.int64
    assert torch.equal(ei, sc[:, :2].long().t())
    assert torch.equal(w.view(torch.int64), sc[:, 2].contiguous().view(torch.int64))
    assert torch.equal(eptr.cpu(), torch.as_tensor(ptr).cpu())
    assert ops.last_stats["entries"] == sc.shape[0] and ops.last_stats["host_syncs"] == HOST_SYNCS
    ei1, w1, _ = ops.snapshot_gcn_norm(sc, ptr, n, add_self_loops=False, normalize=False)
    assert torch.equal(ei1, ei) and w1.dtype == torch.float32 and bool((w1 == 1).all())


@pytest.mark.parametrize("kw", [{"fill_value": 2.0}, {"fill_value": 2.0, "weighted": True}, {"add_self_loops": False},
                                {"add_self_loops": False, "weighted": True}, {"normalize": False}, {"normalize": False, "weighted": True}])
def test_fill_value_and_switches(ops, kw):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    ei, val, eptr = check_call(ops, sc, ptr, n, f"{kw}", **kw)
    if kw.get("fill_value") == 2.0:
        p, e = ptr.tolist(), eptr.tolist()
        present = torch.zeros(n, dtype=torch.bool, device="cuda")
        present[sc[p[0]:p[1], :2].long().reshape(-1)] = True
        loops = val[e[1] - n:e[1]][~present]                 # dis * 2 * dis with dis = 2^-1/2: within the bound of 1
        assert bool(((loops - 1.0).abs() <= 16 * U).all())


# ------------------------------------------------------------------------------------------------ 2. batches, larger num_nodes
@pytest.mark.parametrize("weighted", [False, True])
def test_node_ptr_batch_with_views_and_depths(ops, weighted):
    sizes = [100, 65, 63, 1, 64, 129]
    n, sc, ptr, node_ptr = batch_snapshots(ops, sizes)
    G = len(sizes)
    ei, val, eptr = check_call(ops, sc, ptr, n, f"batch weighted={weighted}", node_ptr=node_ptr, weighted=weighted)
    p, e = ptr.tolist(), eptr.tolist()
    for s in range(len(p) - 1):
        g = s % G
        lo, hi = node_ptr[g], node_ptr[g + 1]
        seg = ei[:, e[s]:e[s + 1]]
        assert e[s + 1] - e[s] == p[s + 1] - p[s] + sizes[g]
        assert int(seg.min()) >= lo and int(seg.max()) < hi                  # loops only inside the graph's range
        assert torch.equal(seg[0, -sizes[g]:], torch.arange(lo, hi, device="cuda"))
        part = sc[p[s]:p[s + 1]].clone()                                     # the segment alone, as a graph of its own size
        part[:, :2] -= lo
        a_ei, a_val, _ = ops.snapshot_gcn_norm(part, [0, part.shape[0]], sizes[g], weighted=weighted, dtype=torch.float64)
        assert torch.equal(a_ei + lo, seg) and torch.equal(a_val.view(torch.int64), val[e[s]:e[s + 1]].view(torch.int64)), f"segment {s}"


def test_num_nodes_larger_than_the_eliminations(ops):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "degree", [n // 8, n // 4, n // 2])
    ei, val, eptr = check_call(ops, sc, ptr, n + 37, "num_nodes + 37", weighted=True)
    e = eptr.tolist()
    assert e[-1] == sc.shape[0] + 6 * (n + 37)
    assert bool((val[e[1] - 37:e[1]] == 1.0).all()) and torch.equal(ei[1, e[1] - 37:e[1]], torch.arange(n, n + 37, device="cuda"))


def test_all_but_one_removed_empty_segments_and_no_rows(ops):
    n = 600
    sc, ptr = depths_views(ops, n, 3, 6, "random", [n // 2, n - 1], views=1)
    p = ptr.tolist()
    assert p[2] == p[1], "removing all but one vertex leaves no row"
    check_call(ops, sc, ptr, n, "n - 1 removed")
    check_call(ops, sc, [0, 0] + p[1:] + [p[-1]], n, "empty segments first and last", weighted=True)
    empty = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    ei, val, eptr = check_call(ops, empty, [0, 0, 0], 5, "m = 0")
    assert ei.tolist() == [[0, 1, 2, 3, 4] * 2] * 2 and bool((val == 1).all()) and eptr.tolist() == [0, 5, 10]
    ei, val, eptr = ops.snapshot_gcn_norm(empty, [0, 0], 5, add_self_loops=False)
    assert ei.shape == (2, 0) and val.numel() == 0 and eptr.tolist() == [0, 0]
    ei, val, eptr = ops.snapshot_gcn_norm(empty, [0, 0], 0)
    assert ei.shape == (2, 0) and eptr.tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 3. inputs with loop rows
HAND = [[1, 0, 0.5], [0, 0, 3.0], [2, 0, 0.25], [0, 0, 4.0],     # two loop rows of id 0 with different weights: the last wins
        [0, 1, 0.5],
        [0, 2, 0.25], [2, 2, 7.0],
        [5, 5, 2.0]]                                              # an id with nothing but a loop row


@pytest.mark.parametrize("weighted", [False, True])
def test_hand_built_input_with_loop_rows(ops, weighted):
    rows = torch.tensor(HAND, dtype=torch.float64).cuda()
    ei, val, eptr = check_call(ops, rows, [0, 8], 7, f"hand-built weighted={weighted}", weighted=weighted)
    assert ops.last_stats["loops_removed"] == 4 and ops.last_stats["entries"] == 8 - 4 + 7 and ei.shape == (2, 11)
    assert ei[:, :4].tolist() == [[1, 2, 0, 0], [0, 0, 1, 2]] and ei[0, 4:].tolist() == list(range(7))
    _, w, _ = ops.snapshot_gcn_norm(rows, [0, 8], 7, weighted=weighted, normalize=False, dtype=torch.float64)
    assert w[4:].tolist() == ([4.0, 1.0, 7.0, 1.0, 1.0, 2.0, 1.0] if weighted else [1.0] * 7)
    # two segments (the second one's offsets depend on the loop rows in front of it), and the rows kept as they are
    two = torch.cat([rows, rows])
    ei2, val2, eptr2 = check_call(ops, two, [0, 8, 16], 7, "hand-built twice", weighted=weighted)
    assert eptr2.tolist() == [0, 11, 22] and ops.last_stats["loops_removed"] == 8
    assert torch.equal(ei2[:, 11:], ei) and torch.equal(val2[11:].view(torch.int64), val.view(torch.int64))
    check_call(ops, two, [0, 8, 16], 7, "hand-built, loops kept", weighted=weighted, add_self_loops=False)
    assert ops.last_stats["loops_removed"] == 0 and ops.last_stats["entries"] == 16
    check_call(ops, two, [0, 0, 8, 8, 16, 16], 7, "hand-built with empty segments", weighted=weighted, fill_value=2.0)


def test_loop_rows_across_tiles(ops):
    """An elimination result with loop rows put into it: one behind the first row of every 7th block, a second one with another
    weight at the end of every 21st -- loop rows in most 1,024-row tiles, segment starts off the tile grid."""
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    rows, p = sc.cpu().numpy(), ptr.tolist()
    out, new_ptr = [], [0]
    for s in range(6):
        part = rows[p[s]:p[s + 1]]
        starts = np.flatnonzero(np.r_[True, part[1:, 1] != part[:-1, 1]])
        ends = np.r_[starts[1:], len(part)]
        pos, ins = [], []
        for b, (a, z) in enumerate(zip(starts, ends)):
            c = part[a, 1]
            if b % 7 == 0:
                pos.append(a + 1), ins.append([c, c, 0.5 + b])
            if b % 21 == 0:
                pos.append(z), ins.append([c, c, 0.25 + b])
        part = np.insert(part, pos, np.array(ins), axis=0)
        out.append(part)
        new_ptr.append(new_ptr[-1] + len(part))
    sc2 = torch.from_numpy(np.concatenate(out)).cuda()
    assert sc2.shape[0] > 8 * 1024
    for weighted in (False, True):
        check_call(ops, sc2, new_ptr, n, f"loop rows in every tile, weighted={weighted}", weighted=weighted)
        assert ops.last_stats["loops_removed"] == sc2.shape[0] - sc.shape[0]
    check_call(ops, sc2[1:], [0] + [v - 1 for v in new_ptr[1:]], n, "odd start", weighted=True)   # rows off the 16-byte grid


# ------------------------------------------------------------------------------------------------ 4. errors
def test_errors_leave_the_handle_intact(ops):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    p = ptr.tolist()
    shuffled = sc.clone()
    perm = torch.randperm(p[1], generator=torch.Generator().manual_seed(0)).cuda()
    shuffled[:p[1]] = sc[:p[1]][perm]
    with pytest.raises(ValueError, match="contiguous|grouped"):
        ops.snapshot_gcn_norm(shuffled, ptr, n)
    bad = sc.clone()
    bad[5, 0] = n + 3
    with pytest.raises(ValueError, match="range"):
        ops.snapshot_gcn_norm(bad, ptr, n)
    two = torch.tensor([[0, 1, 1.0], [1, 0, 1.0], [3, 4, 1.0], [4, 3, 1.0]], dtype=torch.float64).cuda()
    ok = ops.snapshot_gcn_norm(two, [0, 2, 4], 6, node_ptr=[0, 3, 6])
    assert ok[2].tolist() == [0, 5, 10]
    with pytest.raises(ValueError, match="range"):
        ops.snapshot_gcn_norm(two, [0, 1, 4], 6, node_ptr=[0, 3, 6])          # row (1, 0) in graph 1
    for w in (0.0, -1.0, float("nan"), float("inf")):
        bad = sc.clone()
        bad[7, 2] = w
        with pytest.raises(ValueError):
            ops.snapshot_gcn_norm(bad, ptr, n, weighted=True)
        ops.snapshot_gcn_norm(bad, ptr, n)                                     # unweighted: the weights are not looked at
        if w == w:
            _, v, _ = ops.snapshot_gcn_norm(bad, ptr, n, weighted=True, normalize=False, dtype=torch.float64)
            assert float(v[7]) == w                                            # and without normalize they are only copied
    check_call(ops, sc, ptr, n, "after the errors", weighted=True)


# ------------------------------------------------------------------------------------------------ 5. the adapters
def adapter_pairs(make, g):
    plain, norm = make(False).augment(g), make(True).augment(g)
    flat = lambda x: [x] if not isinstance(x, list) else [z for y in x for z in flat(y)]
    plain, norm = flat(plain), flat(norm)
    assert len(plain) == len(norm)
    return list(zip(plain, norm))


@pytest.mark.parametrize("keep_weights", [False, True])
@pytest.mark.parametrize("which", ["rLap", "rLapViews", "rLapDepths"])
def test_adapters(ops, which, keep_weights):
    from rlap_amd.adapters import Graph, rLap, rLapDepths, rLapViews
    n = 1200
    x = torch.randn(n + 50, 8, generator=torch.Generator().manual_seed(0)).cuda()     # more rows than max id + 1
    g = Graph(x, torch.from_numpy(ba_graph(n, 4, 3)).cuda(), None)
    make = {"rLap": lambda on: rLap(0.3, "random", "asc", keep_weights=keep_weights, seed=8, gcn_norm=on),
            "rLapViews": lambda on: rLapViews((0.3, 0.45), "random", "asc", keep_weights=keep_weights, seed=8, gcn_norm=on),
            "rLapDepths": lambda on: rLapDepths((0.1, 0.3, 0.5), "random", "asc", keep_weights=keep_weights, seed=8, views=2, gcn_norm=on)}[which]
    pairs = adapter_pairs(make, g)
    assert len(pairs) == {"rLap": 1, "rLapViews": 2, "rLapDepths": 6}[which]
    for k, (gp, gn) in enumerate(pairs):
        assert (gp.edge_weights is not None) == keep_weights
        w = gp.edge_weights if keep_weights else torch.ones(gp.edge_index.shape[1], dtype=torch.float64)
        part = torch.cat([gp.edge_index.t().double().cpu(), w.double().cpu()[:, None]], 1)
        src, dst, val = torch_segment(part, 0, n + 50, keep_weights)
        assert gn.x is x and gn.edge_index.dtype == torch.int64 and gn.edge_weights.dtype == torch.float32
        assert torch.equal(gn.edge_index.cpu(), torch.stack([src, dst])), f"{which} view {k}"
        assert_values(gn.edge_weights, val.float(), 2.0 ** -23, f"{which} view {k}")
        assert gn.edge_index.shape[1] == gp.edge_index.shape[1] + n + 50


@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_one_gcn_layer_agrees_with_the_dense_product(ops, o_v):
    """zeros.index_add_(0, ei[1], w[:, None] * h[ei[0]]) in float64 against D^-1/2 (A + I) D^-1/2 @ h, A[target, source] += w and D
    its row sums (the target degrees): sums of at most a few hundred terms of magnitude <= max|h|, so 1e-12 relative in the max norm
    hides nothing and trips on any wrong index or degree."""
    from rlap_amd.adapters import Graph, rLap
    n = 500
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    view = rLap(0.25, o_v, "asc", keep_weights=True, seed=2).augment(g)
    part = torch.cat([view.edge_index.t().double(), view.edge_weights[:, None]], 1)
    ei, w, _ = ops.snapshot_gcn_norm(part, [0, part.shape[0]], n, weighted=True, dtype=torch.float64)
    h = torch.randn(n, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).cuda()
    out = torch.zeros_like(h).index_add_(0, ei[1], w[:, None] * h[ei[0]])
    A = torch.zeros(n, n, dtype=torch.float64, device="cuda")
    A.index_put_((view.edge_index[1], view.edge_index[0]), view.edge_weights, accumulate=True)
    A = A + torch.eye(n, dtype=torch.float64, device="cuda")
    dis = A.sum(1).pow(-0.5)
    ref = (dis[:, None] * A * dis[None, :]) @ h
    err = ((out - ref).abs().max() / ref.abs().max()).item()
    print(f"{o_v}: GCN layer against the dense product, relative max-norm error {err:.3e}")
    assert err <= 1e-12
