"""Propagation plans on the device (ops.snapshot_plan, SnapshotPlan.propagate, adapters.Snapshots.plan).

The contract is bits: a planned call returns what ops.snapshot_propagate returns on the same input with the same flags, so every
comparison below is torch.equal on results of equal dtype and there is no tolerance anywhere.  One combination is pinned
independently of the unplanned call: against the host mirror of rlap_spmm.h (tests/csrc/spmm_mirror.cc) fed with the float64
coefficients of ops.snapshot_gcn_norm.
"""
import numpy as np
import pytest
import torch

import spmm_mirror
from util import ba_graph

pytestmark = pytest.mark.gpu

ALL_F = (1, 3, 16, 64, 200, 260)   # 260 float32 columns and 200 float64 columns take more than one group of lanes per row
LIST_KW = ("weighted", "add_self_loops", "fill_value", "normalize")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return spmm_mirror.build(tmp_path_factory.mktemp("spmm"))


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def features(n, F, layers=None, seed=0, dtype=torch.float64):
    shape = (n, F) if layers is None else (layers, n, F)
    g = torch.Generator().manual_seed(1000 * F + seed + (7 if layers else 0))
    x = torch.randn(shape, dtype=torch.float64, generator=g) * (10.0 ** torch.randint(-2, 3, shape, generator=g).double())
    return x.to(dtype).cuda()


def depths_views(ops, n, m, seed, o_v, ts, views=2, node_ptr=None):
    ei = torch.from_numpy(ba_graph(n, m, seed)).cuda()
    return ops.approximate_cholesky_depths(ei, None, n, ts, o_v, "asc", views=views, node_ptr=node_ptr, seed=11, return_device="same")


def layers_of(ptr, node_ptr):
    S = len(torch.as_tensor(ptr).tolist()) - 1
    return S // (len(node_ptr) - 1 if node_ptr is not None else 1)


def check_plan(ops, sc, ptr, n, what, node_ptr=None, Fs=(3, 64), dtypes=(torch.float64, torch.float32), plan=None, **kw):
    """One plan with both directions against the unplanned call: every F of Fs, both dtypes, both x forms, both directions.
    Returns the plan."""
    if plan is None:
        plan = ops.snapshot_plan(sc, ptr, n, node_ptr=node_ptr, **kw)
        assert ops.last_stats["host_syncs"] == 1, what
    L = layers_of(ptr, node_ptr)
    assert (plan.layers, plan.num_nodes, plan.directions) == (L, n, "both")
    for F in Fs:
        for dtype in dtypes:
            for per_layer in (False, True):
                x = features(n, F, L if per_layer else None, dtype=dtype)
                for transpose in (False, True):
                    tag = f"{what} F={F} {dtype} {'per-layer' if per_layer else 'shared'} {'T' if transpose else 'N'}"
                    y = plan.propagate(x, transpose=transpose)
                    assert ops.last_stats["host_syncs"] == 0, tag
                    ref = ops.snapshot_propagate(sc, ptr, n, x, node_ptr=node_ptr, transpose=transpose, **kw)
                    assert y.is_cuda and y.is_contiguous() and same(y, ref), f"{tag}: differs from the unplanned call"
                    assert plan.entries == ops.last_stats["entries"], tag
    return plan


def mirror_result(ops, mirror, sc, ptr, n, x, transpose, **kw):
    """The host mirror fed with the float64 coefficients of ops.snapshot_gcn_norm of the same flags (one graph per layer)."""
    ei, val, eptr = ops.snapshot_gcn_norm(sc, ptr, n, dtype=torch.float64, **kw)
    ei, val, e = ei.cpu().numpy(), val.cpu().numpy(), eptr.tolist()
    x = x.detach().cpu().double().numpy()
    out = np.zeros((len(e) - 1, n, x.shape[-1]))
    for s in range(len(e) - 1):
        out[s] = spmm_mirror.entries(mirror, ei[0, e[s]:e[s + 1]], ei[1, e[s]:e[s + 1]], val[e[s]:e[s + 1]], n, x[s] if x.ndim == 3 else x,
                                     kw.get("add_self_loops", True), transpose)
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------ 1. equality with the unplanned call
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_depths_views_equal_the_unplanned_call(ops, mirror, o_v, weighted):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, o_v, [n // 8, n // 4, n // 2])
    assert ptr.numel() == 7
    plan = check_plan(ops, sc, ptr, n, f"{o_v} weighted={weighted}", Fs=ALL_F, weighted=weighted)
    assert plan.info["blocks"] == int(ops.snapshot_stats(sc, ptr, n)["nodes"].sum()) and plan.info["loops_removed"] == 0
    # pinned independently of the unplanned call: the host mirror with the coefficients of snapshot_gcn_norm
    for transpose in (False, True):
        x = features(n, 16, 6, seed=3)
        want = mirror_result(ops, mirror, sc, ptr, n, x, transpose, weighted=weighted)
        assert same(plan.propagate(x, transpose=transpose).cpu(), want), f"{o_v} {weighted} T={transpose}: differs from the host mirror"


# ------------------------------------------------------------------------------------------------ 2. switches
@pytest.mark.parametrize("kw", [{"fill_value": 2.0}, {"fill_value": 2.0, "weighted": True}, {"add_self_loops": False},
                                {"add_self_loops": False, "weighted": True}, {"normalize": False}, {"normalize": False, "weighted": True},
                                {"add_self_loops": False, "normalize": False}, {"add_self_loops": False, "normalize": False, "weighted": True}])
def test_fill_value_and_switches(ops, kw):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    check_plan(ops, sc, ptr, n, f"{kw}", **kw)


# ------------------------------------------------------------------------------------------------ 3. shapes the indexing can get wrong
@pytest.mark.parametrize("weighted", [False, True])
def test_node_ptr_batch_of_unequal_graphs(ops, weighted):
    sizes, views = [100, 65, 63, 1, 64, 129], 2
    node_ptr = [0] + [int(v) for v in np.cumsum(sizes)]
    parts = [ba_graph(k, 3, 40 + g) + node_ptr[g] for g, k in enumerate(sizes) if k >= 4]
    ei = torch.from_numpy(np.concatenate(parts, 1)).cuda()
    n = node_ptr[-1]
    ts = torch.tensor([[[k // 4 for k in sizes]] * views, [[k // 2 for k in sizes]] * views])
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, ts, "random", "asc", node_ptr=node_ptr, views=views, seed=4, return_device="same")
    assert ptr.numel() == 2 * views * len(sizes) + 1
    plan = check_plan(ops, sc, ptr, n, f"batch weighted={weighted}", node_ptr=node_ptr, Fs=(1, 16, 200), weighted=weighted)
    assert plan.layers == 4


def test_num_nodes_larger_than_the_eliminations(ops):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "degree", [n // 8, n // 4, n // 2])
    plan = check_plan(ops, sc, ptr, n + 37, "num_nodes + 37", weighted=True)
    x = features(n + 37, 3)
    assert same(plan.propagate(x)[:, n:], x[n:].expand(6, 37, 3))            # trailing ids: their loop alone, coefficient 1
    check_plan(ops, sc, ptr, n + 37, "num_nodes + 37, no loops", weighted=True, add_self_loops=False)


def test_all_but_one_removed_empty_segments_and_no_rows(ops):
    n = 600
    sc, ptr = depths_views(ops, n, 3, 6, "random", [n // 2, n - 1], views=1)
    p = ptr.tolist()
    assert p[2] == p[1], "removing all but one vertex leaves no row"
    check_plan(ops, sc, ptr, n, "n - 1 removed")
    check_plan(ops, sc, [0, 0] + p[1:] + [p[-1]], n, "empty segments in the middle and at the end", weighted=True)
    check_plan(ops, sc, [0, p[1], p[1], p[1], p[2]], n, "empty segments in the middle", weighted=True)
    empty = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    plan = check_plan(ops, empty, [0, 0, 0], 5, "m = 0")
    x = features(5, 3)
    assert same(plan.propagate(x), x.expand(2, 5, 3)) and plan.entries == 10          # the loop term alone
    plan = check_plan(ops, empty, [0, 0], 5, "m = 0 without loops", add_self_loops=False)
    assert bool((plan.propagate(x) == 0).all()) and plan.entries == 0
    assert ops.snapshot_plan(empty, [0, 0], 0).propagate(torch.zeros(0, 4).cuda()).shape == (1, 0, 4)


# ------------------------------------------------------------------------------------------------ 4. long lists
def star(leaves, seed, loops=()):
    """A star with centre 0 as an elimination result lays it out: the centre's column block (one row per leaf), then one block
    per leaf.  `loops`: (position in the centre's block, weight) of loop rows (0, 0, w) put into it."""
    rs = np.random.RandomState(seed)
    w = rs.rand(leaves) + 0.5
    centre = [[i + 1, 0, w[i]] for i in range(leaves)]
    for pos, lw in sorted(loops, reverse=True):
        centre.insert(pos, [0, 0, lw])
    rows = centre + [[0, i + 1, w[i] * (1.0 + 2.0 ** -50 * (i % 3))] for i in range(leaves)]   # pairs equal only up to the last bits
    return np.array(rows, dtype=np.float64)


def two_stars(leaves):
    a, b = star(leaves, 1), star(leaves, 2)
    return torch.from_numpy(np.concatenate([a, b])).cuda(), [0, len(a), len(a) + len(b)], leaves + 1


@pytest.mark.parametrize("weighted", [False, True])
def test_star_longer_than_two_chunks(ops, mirror, weighted):
    C = mirror.spmm_chunk()
    sc, ptr, n = two_stars(2 * C + 40)
    plan = check_plan(ops, sc, ptr, n, f"star weighted={weighted}", Fs=ALL_F, weighted=weighted)
    assert plan.info["chunked_lists_forward"] == 2 and plan.info["chunked_lists_transposed"] == 2
    assert plan.desc.chunks_forward == 6 and plan.desc.chunks_transposed == 6
    for t in (False, True):                                                    # the unplanned calls count the same lists
        ops.snapshot_propagate(sc, ptr, n, features(n, 3), weighted=weighted, transpose=t)
        assert ops.last_stats["chunked_lists"] == plan.info["chunked_lists_transposed" if t else "chunked_lists_forward"]
    exact = torch.from_numpy(star(C, 3)).cuda()                                # a list of exactly C entries is not chunked
    plan = check_plan(ops, exact, [0, 2 * C], C + 1, "star of C leaves", Fs=(3,), weighted=weighted)
    assert plan.info["chunked_lists_forward"] == 0 and plan.desc.chunks_transposed == 0
    one_more = torch.from_numpy(star(C + 1, 3)).cuda()
    plan = check_plan(ops, one_more, [0, 2 * C + 2], C + 2, "star of C + 1 leaves", Fs=(3,), weighted=weighted)
    assert plan.info["chunked_lists_forward"] == 1 and plan.desc.chunks_forward == 2


@pytest.mark.parametrize("limit", [0, 4, 5])
def test_chunk_sums_past_their_budget(ops, mirror, limit):
    """The test hook lets a call keep `limit` chunk sums: two stars of three chunks each, so none, the first list's, or the first
    list's and part of the second's fit.  The lists past the budget are summed chunk by chunk by their own group: the same bits."""
    C = mirror.spmm_chunk()
    sc, ptr, n = two_stars(2 * C + 40)
    plan = ops.snapshot_plan(sc, ptr, n, weighted=True)
    x = features(n, 16, 2)
    ref = [ops.snapshot_propagate(sc, ptr, n, x, weighted=True, transpose=t) for t in (False, True)]
    try:
        ops.debug_set_limits(scratch_entries=limit)
        for t in (False, True):
            assert same(plan.propagate(x, transpose=t), ref[t]), f"limit {limit} transpose {t}"
            assert ops.last_stats["host_syncs"] == 0
        check_plan(ops, sc, ptr, n, f"star, {limit} chunk sums kept", Fs=(3, 200), plan=plan, weighted=True)
    finally:
        ops.debug_set_limits()


# ------------------------------------------------------------------------------------------------ 5. dropped loop rows
HAND = [[1, 0, 0.5], [0, 0, 3.0], [2, 0, 0.25], [0, 0, 4.0],     # two loop rows of id 0 with different weights: the last wins
        [0, 1, 0.5],
        [0, 2, 0.25], [2, 2, 7.0],
        [5, 5, 2.0]]                                              # an id with nothing but a loop row


@pytest.mark.parametrize("weighted", [False, True])
def test_star_with_loop_rows(ops, mirror, weighted):
    """Loop rows inside a long block: an entry's place in its list is no longer its place in its block."""
    C = mirror.spmm_chunk()
    leaves = 2 * C + 40
    a = star(leaves, 4, loops=[(3, 2.5), (C, 0.75), (C + 20, 1.25)])
    extra = np.array([[1, 1, 3.0]])                                          # a leaf's loop row, at the end of its block
    a = np.concatenate([a[:leaves + 3 + 1], extra, a[leaves + 3 + 1:]])
    sc = torch.from_numpy(np.concatenate([a, star(leaves, 5)])).cuda()
    ptr, n = [0, len(a), len(a) + 2 * leaves], leaves + 3
    plan = check_plan(ops, sc, ptr, n, f"star with loop rows weighted={weighted}", Fs=(1, 3, 64), weighted=weighted)
    assert plan.info["loops_removed"] == 4 and plan.entries == 4 * leaves + 2 * n
    assert plan.info["chunked_lists_forward"] == 2 and plan.info["chunked_lists_transposed"] == 2
    assert plan.desc.entries_forward == 4 * leaves and plan.desc.entries_transposed == 4 * leaves
    plan = check_plan(ops, sc, ptr, n, "star, loop rows kept", Fs=(3,), weighted=weighted, add_self_loops=False)
    assert plan.info["loops_removed"] == 0 and plan.entries == sc.shape[0]
    short = torch.from_numpy(star(C, 6, loops=[(5, 2.0)])).cuda()             # C + 1 rows of which one is a loop row: one chunk
    plan = check_plan(ops, short, [0, 2 * C + 1], C + 1, "C entries and a loop row", Fs=(3,), weighted=weighted)
    assert plan.info["chunked_lists_forward"] == 0 and plan.info["loops_removed"] == 1


@pytest.mark.parametrize("weighted", [False, True])
def test_hand_built_input_with_loop_rows(ops, weighted):
    rows = torch.tensor(HAND, dtype=torch.float64).cuda()
    plan = check_plan(ops, rows, [0, 8], 7, f"hand-built weighted={weighted}", weighted=weighted)
    assert plan.info["loops_removed"] == 4 and plan.entries == 8 - 4 + 7
    two = torch.cat([rows, rows])
    check_plan(ops, two, [0, 8, 16], 7, "hand-built twice", weighted=weighted)
    check_plan(ops, two, [0, 8, 16], 7, "hand-built, loops kept", weighted=weighted, add_self_loops=False)
    check_plan(ops, two, [0, 0, 8, 8, 16, 16], 7, "hand-built with empty segments", weighted=weighted, fill_value=2.0)
    check_plan(ops, two, [0, 8, 16], 7, "hand-built, weights as they are", weighted=weighted, normalize=False)


# ------------------------------------------------------------------------------------------------ 6. independence
def test_plan_does_not_depend_on_buffers_poison_or_the_rows(ops):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    sc = sc.clone()
    x = features(n, 16)
    ref = [ops.snapshot_propagate(sc, ptr, n, x, weighted=True, transpose=t) for t in (False, True)]
    try:
        for byte in (0xFF, 0x00, 0x5A):   # the poison fills the arena, the result and -- before the build -- the whole plan buffer
            ops.debug_set_poison(byte)
            plan = ops.snapshot_plan(sc, ptr, n, weighted=True)
            for t in (False, True):
                assert same(plan.propagate(x, transpose=t), ref[t]), f"poison {byte:#x}"
    finally:
        ops.debug_set_poison(-1)
    ops.snapshot_ppr(sc, ptr, n)                                             # another call dirties the arena between two uses
    for t in (False, True):
        assert same(plan.propagate(x, transpose=t), ref[t])
    sc.zero_()                                                               # the rows are gone: the plan does not read them
    for t in (False, True):
        assert same(plan.propagate(x, transpose=t), ref[t])


# ------------------------------------------------------------------------------------------------ 7. accounting
def test_accounting_and_directions(ops):
    import ctypes
    from rlap_amd import _lib
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    x = features(n, 16)
    both = ops.snapshot_plan(sc, ptr, n)
    st = dict(ops.last_stats)
    assert st["host_syncs"] == 1 and st["entries"] == sc.shape[0] + 6 * n and st["loops_removed"] == 0 and st["arena_bytes"] > 0
    assert set(st) == {"entries", "blocks", "chunked_lists_forward", "chunked_lists_transposed", "loops_removed", "arena_bytes", "host_syncs"}
    bound = ctypes.c_size_t()
    flags = _lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE
    assert _lib.load().rlap_snapshot_plan_bytes(sc.shape[0], 6, 1, n, flags, ctypes.byref(bound)) == 0
    assert 0 < both.nbytes <= bound.value and both.nbytes == both.buffer.numel() and both.buffer.dtype == torch.uint8
    assert both.nbytes >= 2 * 16 * sc.shape[0] and both.entries == st["entries"] and both.directions == "both"
    for t in (False, True):
        both.propagate(x, transpose=t)
        assert ops.last_stats["host_syncs"] == 0
    fwd = ops.snapshot_plan(sc, ptr, n, directions="forward")
    assert ops.last_stats["chunked_lists_transposed"] == -1 and fwd.directions == "forward" and fwd.nbytes <= both.nbytes
    assert same(fwd.propagate(x), both.propagate(x))
    with pytest.raises(ValueError, match="forward"):
        fwd.propagate(x, transpose=True)
    with pytest.raises(ValueError, match="forward"):
        fwd.propagate(x.clone().requires_grad_(True))                         # the backward pass would need the other direction
    tr = ops.snapshot_plan(sc, ptr, n, directions="transposed")
    assert tr.nbytes <= both.nbytes and same(tr.propagate(x, transpose=True), both.propagate(x, transpose=True))
    with pytest.raises(ValueError, match="transposed"):
        tr.propagate(x)
    with pytest.raises(ValueError, match="directions"):
        ops.snapshot_plan(sc, ptr, n, directions="backward")
    with pytest.raises(ValueError, match="rows"):
        both.propagate(features(n + 1, 3))


# ------------------------------------------------------------------------------------------------ 8. autograd
@pytest.mark.parametrize("per_layer", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gradient_equals_the_unplanned_calls(ops, per_layer, dtype):
    n, F = 500, 16
    sc, ptr = depths_views(ops, n, 3, 5, "random", [n // 4, n // 2])
    L = ptr.numel() - 1
    plan = ops.snapshot_plan(sc, ptr, n, weighted=True)
    x0 = features(n, F, L if per_layer else None, seed=3, dtype=dtype)
    z = features(n, F, L, seed=4, dtype=dtype)
    for transpose in (False, True):
        xa, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
        ya = plan.propagate(xa, transpose=transpose)
        yb = ops.snapshot_propagate(sc, ptr, n, xb, weighted=True, transpose=transpose)
        assert ya.requires_grad and same(ya.detach(), yb.detach())
        (ya * z).sum().backward()
        assert ops.last_stats["host_syncs"] == 0
        (yb * z).sum().backward()
        assert xa.grad.shape == x0.shape and same(xa.grad, xb.grad), f"per_layer={per_layer} {dtype} T={transpose}"
    with torch.no_grad():
        assert not plan.propagate(x0.clone().requires_grad_(True)).requires_grad


def test_conv_on_planned_snapshots_and_no_double_backward(ops):
    from rlap_amd.adapters import Graph, PlannedSnapshots, SnapshotGCNConv, rLapViews
    n, cin, cout = 500, 8, 5
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    snaps = rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2).snapshots(g)
    planned = snaps.plan()
    assert isinstance(planned, PlannedSnapshots) and planned.layers == snaps.layers == 2 and planned.snapshot_plan is None
    torch.manual_seed(3)
    conv = SnapshotGCNConv(cin, cout).double().cuda()
    with torch.no_grad():
        conv.bias.copy_(torch.randn(cout))
    z = features(n, cout, 2, seed=7)
    got = []
    for holder in (planned, snaps):
        conv.zero_grad()
        x = features(n, cin, seed=6).requires_grad_(True)
        out = conv(x, holder)
        (out * z).sum().backward()
        got.append((out.detach(), conv.weight.grad.clone(), conv.bias.grad.clone(), x.grad.clone()))
    for what, a, b in zip(("output", "grad W", "grad b", "grad x"), *got):
        assert same(a, b), what
    first = planned.snapshot_plan
    assert first is not None and same(planned.propagate(z[0], transpose=True), snaps.propagate(z[0], transpose=True))
    assert planned.snapshot_plan is first                                    # built once
    x = features(n, 3).requires_grad_(True)
    (gr,) = torch.autograd.grad(planned.propagate(x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        gr.sum().backward()


# ------------------------------------------------------------------------------------------------ 9. errors
def test_errors_leave_the_handle_intact(ops):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    p = ptr.tolist()
    shuffled = sc.clone()
    perm = torch.randperm(p[1], generator=torch.Generator().manual_seed(0)).cuda()
    shuffled[:p[1]] = sc[:p[1]][perm]
    out_of_range = sc.clone()
    out_of_range[5, 0] = n + 3
    weight = sc.clone()
    weight[7, 2] = -1.0
    for bad, kw, match in ((shuffled, {}, "contiguous|grouped"), (out_of_range, {}, "range"), (weight, {"weighted": True}, "rlap")):
        with pytest.raises(ValueError, match=match):
            ops.snapshot_plan(bad, ptr, n, **kw)
        check_plan(ops, sc, ptr, n, f"after {match}", Fs=(16,), dtypes=(torch.float64,), weighted=True)
    ops.snapshot_plan(weight, ptr, n)                                        # unweighted: the weights are not looked at


# ------------------------------------------------------------------------------------------------ 10. streams
def test_planned_call_on_a_side_stream(ops):
    """The planned call never synchronises: what orders it behind the kernels that produce x, and in front of those that consume y,
    is the stream the handle is bound to at the call.  The plan is built on the default stream; on a side stream that has waited for
    it, x comes out of a chain of torch kernels long enough for the device to lag behind the host, the planned call follows at
    once, and y is consumed there.  The bits of the same calls on the default stream, made after everything has finished."""
    n, F = 3000, 16
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    plan = ops.snapshot_plan(sc, ptr, n, weighted=True)
    base = features(n, F, 6, seed=9, dtype=torch.float32)
    w = torch.randn(2048, 2048, generator=torch.Generator().manual_seed(1)).cuda() / 32.0
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(40):
            w = torch.sin(w @ w)
        x = base + w[:1, :F]                                                  # the last kernel of the chain writes x
        got = []
        for t in (False, True):
            y = plan.propagate(x, transpose=t)
            assert ops.last_stats["host_syncs"] == 0
            got.append(y * 2.0)                                                # consumed on the same stream
    side.synchronize()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(x).all()) and not torch.equal(x, base)
    for t in (False, True):
        ref = plan.propagate(x, transpose=t) * 2.0
        assert same(got[t], ref), f"transpose={t}: the side stream's result differs from the default stream's"
        assert same(plan.propagate(x, transpose=t), ops.snapshot_propagate(sc, ptr, n, x, weighted=True, transpose=t))
