"""GCN propagation of snapshots on the device (ops.snapshot_propagate, rlap_snapshot_propagate), its gradient and the adapters built
on it (Snapshots, SnapshotGCNConv).

1. The yardstick is independent of the code under test: the torch formulation of tests/test_gpu_gcn_norm.py restated below (PyG's
   gcn_norm; PyG itself is not installed), per segment, float64 on the CPU, followed by zeros.index_add_(0, dst, val[:, None] *
   x[src]) -- src / dst swapped for the transposed product.  Per output element |y - ref| <= (16 + 4 L) u A, u = 2^-53,
   A = sum |c_e| |x_e| from the yardstick, L = the longest list of the call (and the longest column block, which the degrees are
   summed over: for the symmetric patterns of elimination results the two are one number) plus one.  Derived, not measured:
   (16 + 2 L) u is the relative bound of a coefficient established in tests/test_gpu_gcn_norm.py; every product is rounded once on
   each side (inside the 16); a sum of at most L terms carries (L - 1) u on each side, whatever its order.  Unweighted degrees are
   exact integers: (16 + 2 L) u.  An id without entries gets exactly 0.
2. Bit for bit: the float64 result equals the host mirror (tests/csrc/spmm_mirror.cc around rlap_amd/csrc/rlap_spmm.h, the header
   the kernels include) fed with the float64 coefficients of ops.snapshot_gcn_norm of the same flags; the float32 result equals
   the float64 result of the same features rounded once; twice the same call, per-segment calls and a poisoned arena give the
   same bits.
"""
import math

import numpy as np
import pytest
import torch

import spmm_mirror
from util import ba_graph

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
HOST_SYNCS = 1
ALL_F = (1, 3, 16, 64, 200)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return spmm_mirror.build(tmp_path_factory.mktemp("spmm"))


# ------------------------------------------------------------------------------------------------ the yardstick
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


def flags_of(kw):
    return {"weighted": kw.get("weighted", False), "add_self_loops": kw.get("add_self_loops", True), "fill": kw.get("fill_value", 1.0),
            "normalize": kw.get("normalize", True)}


def segments(ptr, num_nodes, node_ptr):
    """[(s, layer, lo, hi, r0, r1)] of a call."""
    p = torch.as_tensor(ptr).tolist()
    G = len(node_ptr) - 1 if node_ptr is not None else 1
    out = []
    for s in range(len(p) - 1):
        lo, hi = (int(node_ptr[s % G]), int(node_ptr[s % G + 1])) if node_ptr is not None else (0, num_nodes)
        out.append((s, s // G, lo, hi, p[s], p[s + 1]))
    return out


def yardstick(sc, ptr, n, x, node_ptr=None, transpose=False, **kw):
    """(ref, A, count, longest): the product, sum |c| |x| and the entries per output row, each (layers, n, F) / (layers, n), and the
    longest list or column block of the call."""
    x = x.detach().cpu().double()
    segs = segments(ptr, n, node_ptr)
    L = segs[-1][1] + 1
    F = x.shape[-1]
    ref, A = torch.zeros(L, n, F, dtype=torch.float64), torch.zeros(L, n, F, dtype=torch.float64)
    count = torch.zeros(L, n, dtype=torch.int64)
    longest = 0
    for s, l, lo, hi, r0, r1 in segs:
        src, dst, val = torch_segment(sc[r0:r1], lo, hi, **flags_of(kw))
        xl = x[l] if x.dim() == 3 else x
        for key in (src, dst):                                          # lists by source and column blocks alike, loops apart
            k = key[src != dst] if kw.get("add_self_loops", True) else key
            if k.numel():
                longest = max(longest, int(torch.bincount(k).max()))
        if transpose:
            src, dst = dst, src
        ref[l].index_add_(0, dst, val[:, None] * xl[src])
        A[l].index_add_(0, dst, val.abs()[:, None] * xl[src].abs())
        count[l].index_add_(0, dst, torch.ones_like(dst))
    return ref, A, count, longest


def bound_factor(longest, weighted):
    L = longest + 1
    return (16 + 4 * L) * U if weighted else (16 + 2 * L) * U


def assert_close(y, ref, A, count, factor, what):
    y = y.detach().cpu().double()
    assert y.shape == ref.shape, f"{what}: {tuple(y.shape)} vs {tuple(ref.shape)}"
    assert bool(torch.isfinite(y).all()), f"{what}: a value is not finite"
    empty = count == 0
    assert bool((y[empty] == 0).all()), f"{what}: an id without entries is not exactly 0"
    err = (y - ref).abs()
    ratio = (err / A.clamp_min(1e-300))[A > 0]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"{what}: max |y - ref| / A = {worst:.3e} (bound {factor:.3e})")
    assert bool((err <= factor * A).all()), f"{what}: error {worst:.3e} A above {factor:.3e} A"
    return worst


def mirror_result(ops, mirror, sc, ptr, n, x, node_ptr=None, transpose=False, **kw):
    """The host mirror fed with the float64 coefficients of ops.snapshot_gcn_norm of the same flags."""
    ei, val, eptr = ops.snapshot_gcn_norm(sc, ptr, n, node_ptr=node_ptr, dtype=torch.float64, **kw)
    ei, val, e = ei.cpu().numpy(), val.cpu().numpy(), eptr.tolist()
    x = x.detach().cpu().double().numpy()
    segs = segments(ptr, n, node_ptr)
    out = np.zeros((segs[-1][1] + 1, n, x.shape[-1]))
    for s, l, lo, hi, _, _ in segs:
        xl = x[l] if x.ndim == 3 else x
        y = spmm_mirror.entries(mirror, ei[0, e[s]:e[s + 1]], ei[1, e[s]:e[s + 1]], val[e[s]:e[s + 1]], n, xl,
                                kw.get("add_self_loops", True), transpose)
        out[l, lo:hi] = y[lo:hi]
    return torch.from_numpy(out)


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    view = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def features(n, F, layers=None, seed=0):
    shape = (n, F) if layers is None else (layers, n, F)
    g = torch.Generator().manual_seed(1000 * F + seed + (7 if layers else 0))
    return torch.randn(shape, dtype=torch.float64, generator=g) * (10.0 ** torch.randint(-2, 3, shape, generator=g).double())


def check_call(ops, mirror, sc, ptr, n, what, node_ptr=None, Fs=(3, 64), **kw):
    """One configuration: both x forms, forward and transposed, every F of Fs, float64 and float32.  Returns the worst error ratio."""
    weighted = kw.get("weighted", False)
    layers = segments(ptr, n, node_ptr)[-1][1] + 1
    worst = 0.0
    for F in Fs:
        for per_layer in (False, True):
            x = features(n, F, layers if per_layer else None)
            for transpose in (False, True):
                tag = f"{what} F={F} {'per-layer' if per_layer else 'shared'} {'T' if transpose else 'N'}"
                y = ops.snapshot_propagate(sc, ptr, n, x.cuda(), node_ptr=node_ptr, transpose=transpose, **kw)
                st = dict(ops.last_stats)
                assert st["host_syncs"] == HOST_SYNCS
                assert y.dtype == torch.float64 and y.is_cuda and y.shape == (layers, n, F) and y.is_contiguous()
                ref, A, count, longest = yardstick(sc, ptr, n, x, node_ptr=node_ptr, transpose=transpose, **kw)
                worst = max(worst, assert_close(y, ref, A, count, bound_factor(longest, weighted), tag))
                assert st["entries"] == int(count.sum()), tag
                assert same_bits(y, mirror_result(ops, mirror, sc, ptr, n, x, node_ptr=node_ptr, transpose=transpose, **kw)), \
                    f"{tag}: differs from the host mirror"
                y2 = ops.snapshot_propagate(sc, ptr, n, x.cuda(), node_ptr=node_ptr, transpose=transpose, **kw)
                assert same_bits(y2, y), f"{tag}: the same call twice"
                x32 = x.float()
                y32 = ops.snapshot_propagate(sc, ptr, n, x32.cuda(), node_ptr=node_ptr, transpose=transpose, **kw)
                y64 = ops.snapshot_propagate(sc, ptr, n, x32.double().cuda(), node_ptr=node_ptr, transpose=transpose, **kw)
                assert y32.dtype == torch.float32 and same_bits(y32, y64.float()), f"{tag}: float32 is not the float64 sum rounded once"
    return worst


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
def test_depths_views(ops, mirror, o_v, weighted):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, o_v, [n // 8, n // 4, n // 2])
    assert ptr.numel() == 7
    check_call(ops, mirror, sc, ptr, n, f"{o_v} weighted={weighted}", Fs=ALL_F, weighted=weighted)
    assert ops.last_stats["blocks"] == int(ops.snapshot_stats(sc, ptr, n)["nodes"].sum())
    # a views x depths call equals per-segment calls bit for bit, with the shared and the per-layer features
    p = ptr.tolist()
    for F in (3, 64):
        xs, xp = features(n, F).cuda(), features(n, F, 6).cuda()
        for transpose in (False, True):
            ys = ops.snapshot_propagate(sc, ptr, n, xs, weighted=weighted, transpose=transpose)
            yp = ops.snapshot_propagate(sc, ptr, n, xp, weighted=weighted, transpose=transpose)
            for s in range(6):
                part, pp = sc[p[s]:p[s + 1]], [0, p[s + 1] - p[s]]
                assert same_bits(ops.snapshot_propagate(part, pp, n, xs, weighted=weighted, transpose=transpose)[0], ys[s])
                assert same_bits(ops.snapshot_propagate(part, pp, n, xp[s], weighted=weighted, transpose=transpose)[0], yp[s])
                assert same_bits(ops.snapshot_propagate(part, pp, n, xp[s:s + 1], weighted=weighted, transpose=transpose)[0], yp[s])


@pytest.mark.parametrize("kw", [{"fill_value": 2.0}, {"fill_value": 2.0, "weighted": True}, {"add_self_loops": False},
                                {"add_self_loops": False, "weighted": True}, {"normalize": False}, {"normalize": False, "weighted": True},
                                {"add_self_loops": False, "normalize": False, "weighted": True}])
def test_fill_value_and_switches(ops, mirror, kw):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    check_call(ops, mirror, sc, ptr, n, f"{kw}", **kw)


def test_result_does_not_depend_on_buffers_or_poison(ops):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    x = features(n, 16).cuda()
    ref = [ops.snapshot_propagate(sc, ptr, n, x, weighted=True, transpose=t) for t in (False, True)]
    try:
        for byte in (0xFF, 0x00, 0x5A):
            ops.debug_set_poison(byte)
            for t in (False, True):
                assert same_bits(ops.snapshot_propagate(sc, ptr, n, x, weighted=True, transpose=t), ref[t]), f"poison {byte:#x}"
    finally:
        ops.debug_set_poison(-1)
    ops.snapshot_ppr(sc, ptr, n)                                             # another call dirties the arena in between
    for t in (False, True):
        assert same_bits(ops.snapshot_propagate(sc, ptr, n, x, weighted=True, transpose=t), ref[t])


# ------------------------------------------------------------------------------------------------ 2. batches, larger num_nodes
@pytest.mark.parametrize("weighted", [False, True])
def test_node_ptr_batch_with_views_and_depths(ops, mirror, weighted):
    sizes = [100, 65, 63, 1, 64, 129]
    n, sc, ptr, node_ptr = batch_snapshots(ops, sizes)
    check_call(ops, mirror, sc, ptr, n, f"batch weighted={weighted}", node_ptr=node_ptr, Fs=(1, 16, 200), weighted=weighted)
    # the one-vertex graph: nothing but its loop, coefficient exactly 1
    x = features(n, 16).cuda()
    y = ops.snapshot_propagate(sc, ptr, n, x, node_ptr=node_ptr, weighted=weighted)
    lone = node_ptr[3]
    assert y.shape == (4, n, 16) and all(same_bits(y[l, lone], x[lone]) for l in range(4))
    # a graph's segment alone, as a graph of its own size
    p, G = ptr.tolist(), len(sizes)
    for s in (0, 5, 2 * G + 4):
        g, l = s % G, s // G
        lo, hi = node_ptr[g], node_ptr[g + 1]
        part = sc[p[s]:p[s + 1]].clone()
        part[:, :2] -= lo
        alone = ops.snapshot_propagate(part, [0, part.shape[0]], sizes[g], x[lo:hi], weighted=weighted)
        assert same_bits(alone[0], y[l, lo:hi]), f"segment {s}"


def test_num_nodes_larger_than_the_eliminations(ops, mirror):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "degree", [n // 8, n // 4, n // 2])
    check_call(ops, mirror, sc, ptr, n + 37, "num_nodes + 37", weighted=True)
    x = features(n + 37, 3).cuda()
    y = ops.snapshot_propagate(sc, ptr, n + 37, x, weighted=True)
    assert same_bits(y[:, n:], x[n:].expand(6, 37, 3))                       # trailing ids: their loop alone, coefficient 1
    y = ops.snapshot_propagate(sc, ptr, n + 37, x, weighted=True, add_self_loops=False)
    assert bool((y[:, n:] == 0).all())


def test_all_but_one_removed_empty_segments_and_no_rows(ops, mirror):
    n = 600
    sc, ptr = depths_views(ops, n, 3, 6, "random", [n // 2, n - 1], views=1)
    p = ptr.tolist()
    assert p[2] == p[1], "removing all but one vertex leaves no row"
    check_call(ops, mirror, sc, ptr, n, "n - 1 removed")
    check_call(ops, mirror, sc, [0, 0] + p[1:] + [p[-1]], n, "empty segments first and last", weighted=True)
    empty = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    check_call(ops, mirror, empty, [0, 0, 0], 5, "m = 0")
    x = features(5, 3).cuda()
    assert same_bits(ops.snapshot_propagate(empty, [0, 0, 0], 5, x), x.expand(2, 5, 3))
    assert bool((ops.snapshot_propagate(empty, [0, 0], 5, x, add_self_loops=False) == 0).all())
    assert ops.snapshot_propagate(empty, [0, 0], 0, torch.zeros(0, 4).cuda()).shape == (1, 0, 4)


# ------------------------------------------------------------------------------------------------ 3. long lists, loop rows
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


@pytest.mark.parametrize("weighted", [False, True])
def test_star_longer_than_two_chunks(ops, mirror, weighted):
    C = mirror.spmm_chunk()
    leaves = 2 * C + 37
    a, b = star(leaves, 1), star(leaves, 2)
    sc = torch.from_numpy(np.concatenate([a, b])).cuda()
    ptr, n = [0, len(a), len(a) + len(b)], leaves + 1
    check_call(ops, mirror, sc, ptr, n, f"star weighted={weighted}", Fs=ALL_F, weighted=weighted)
    assert ops.last_stats["chunked_lists"] == 2 and ops.last_stats["blocks"] == 2 * n
    # the chunk rule and not one running sum: the centre's row is the mirror's, and a list of exactly C entries is not chunked
    exact = torch.from_numpy(star(C, 3)).cuda()
    ops.snapshot_propagate(exact, [0, 2 * C], C + 1, features(C + 1, 3).cuda(), weighted=weighted)
    assert ops.last_stats["chunked_lists"] == 0
    one_more = torch.from_numpy(star(C + 1, 3)).cuda()
    check_call(ops, mirror, one_more, [0, 2 * C + 2], C + 2, "star of C + 1 leaves", Fs=(3,), weighted=weighted)
    assert ops.last_stats["chunked_lists"] == 1


@pytest.mark.parametrize("limit", [0, 4, 5])
def test_chunk_sums_past_their_budget(ops, mirror, limit):
    """The test hook (scratch_entries of debug_set_limits) lets the call keep `limit` chunk sums: two stars of three chunks each, so
    none, the first list's, or the first list's and part of the second's fit.  The lists past the budget are summed chunk by chunk
    by their own group of lanes: the same bits."""
    C = mirror.spmm_chunk()
    leaves = 2 * C + 37
    a, b = star(leaves, 1), star(leaves, 2)
    sc = torch.from_numpy(np.concatenate([a, b])).cuda()
    ptr, n = [0, len(a), len(a) + len(b)], leaves + 1
    x = features(n, 16, 2).cuda()
    ref = [ops.snapshot_propagate(sc, ptr, n, x, weighted=True, transpose=t) for t in (False, True)]
    try:
        ops.debug_set_limits(scratch_entries=limit)
        for t in (False, True):
            assert same_bits(ops.snapshot_propagate(sc, ptr, n, x, weighted=True, transpose=t), ref[t]), f"limit {limit} transpose {t}"
            assert ops.last_stats["chunked_lists"] == 2
        check_call(ops, mirror, sc, ptr, n, f"star, {limit} chunk sums kept", Fs=(3, 200), weighted=True)
    finally:
        ops.debug_set_limits()


# F_PATHS: the feature widths at which launch_sums takes a lane path that ALL_F leaves out (V = 4 float32 / 2 float64 a lane).
#   65          : the one-column kernels with two tiles of 64 lanes, the second holding one lane (both types)
#   66, 130     : float32 -- no multiple of 4: the one-column kernels with two and three tiles; float64 -- vector lanes: 33 in one
#                 tile, and 65 in two tiles of which the second holds one lane
#   2, 6, 12    : groups of 1, 2, 4, 8 lanes of which some idle (6: 3 of 4 float64 lanes; 12: 3 of 4 float32, 6 of 8 float64), and
#                 the one-column kernels with two and six lanes (float32, 2 and 6)
#   256         : float32 -- exactly one full tile of 64 vector lanes; float64 -- two full tiles
F_PATHS = (2, 6, 12, 65, 66, 130, 256)


@pytest.fixture
def poisoned(ops):
    """y holds NaN patterns before every call: an element that is never written cannot pass by finding an earlier call's result
    in reused memory."""
    ops.debug_set_poison(0xFF)
    yield
    ops.debug_set_poison(-1)


@pytest.mark.parametrize("F", F_PATHS)
def test_lane_paths_depths_views(ops, mirror, poisoned, F):
    n = 300
    sc, ptr = depths_views(ops, n, 3, 2, "random", [75, 150], views=2)
    assert ptr.numel() == 5
    check_call(ops, mirror, sc, ptr, n, f"lane paths F={F}", Fs=(F,), weighted=True)


@pytest.mark.parametrize("limit", [None, 0])
@pytest.mark.parametrize("F", F_PATHS)
def test_lane_paths_long_lists(ops, mirror, poisoned, F, limit):
    """Two stars of three chunks each: the chunk kernel on the same lane paths, and (limit 0: no chunk sum kept) the rows kernel
    summing a long list chunk by chunk itself."""
    C = mirror.spmm_chunk()
    leaves = 2 * C + 40
    a, b = star(leaves, 1), star(leaves, 2)
    sc = torch.from_numpy(np.concatenate([a, b])).cuda()
    ptr, n = [0, len(a), len(a) + len(b)], leaves + 1
    try:
        if limit is not None:
            ops.debug_set_limits(scratch_entries=limit)
        check_call(ops, mirror, sc, ptr, n, f"stars, lane paths F={F} limit={limit}", Fs=(F,), weighted=True)
        assert ops.last_stats["chunked_lists"] == 2
    finally:
        ops.debug_set_limits()


@pytest.mark.parametrize("weighted", [False, True])
def test_star_with_loop_rows(ops, mirror, weighted):
    """Loop rows inside a long block: an entry's place in its list is no longer its place in its block."""
    C = mirror.spmm_chunk()
    leaves = 2 * C + 37
    a = star(leaves, 4, loops=[(3, 2.5), (C, 0.75), (C + 20, 1.25)])
    extra = np.array([[1, 1, 3.0]])                                          # a leaf's loop row, at the end of its block
    a = np.concatenate([a[:leaves + 3 + 1], extra, a[leaves + 3 + 1:]])
    sc = torch.from_numpy(np.concatenate([a, star(leaves, 5)])).cuda()
    ptr, n = [0, len(a), len(a) + 2 * leaves], leaves + 3
    check_call(ops, mirror, sc, ptr, n, f"star with loop rows weighted={weighted}", Fs=(1, 3, 64), weighted=weighted)
    assert ops.last_stats["chunked_lists"] == 2 and ops.last_stats["entries"] == 4 * leaves + 2 * n
    check_call(ops, mirror, sc, ptr, n, "star, loop rows kept", Fs=(3,), weighted=weighted, add_self_loops=False)
    assert ops.last_stats["entries"] == sc.shape[0]
    # C + 1 rows of which one is a loop row: C entries stay, one chunk
    short = torch.from_numpy(star(C, 6, loops=[(5, 2.0)])).cuda()
    check_call(ops, mirror, short, [0, 2 * C + 1], C + 1, "C entries and a loop row", Fs=(3,), weighted=weighted)
    assert ops.last_stats["chunked_lists"] == 0


HAND = [[1, 0, 0.5], [0, 0, 3.0], [2, 0, 0.25], [0, 0, 4.0],     # two loop rows of id 0 with different weights: the last wins
        [0, 1, 0.5],
        [0, 2, 0.25], [2, 2, 7.0],
        [5, 5, 2.0]]                                              # an id with nothing but a loop row


@pytest.mark.parametrize("weighted", [False, True])
def test_hand_built_input_with_loop_rows(ops, mirror, weighted):
    rows = torch.tensor(HAND, dtype=torch.float64).cuda()
    check_call(ops, mirror, rows, [0, 8], 7, f"hand-built weighted={weighted}", weighted=weighted)
    assert ops.last_stats["entries"] == 8 - 4 + 7
    two = torch.cat([rows, rows])
    check_call(ops, mirror, two, [0, 8, 16], 7, "hand-built twice", weighted=weighted)
    check_call(ops, mirror, two, [0, 8, 16], 7, "hand-built, loops kept", weighted=weighted, add_self_loops=False)
    check_call(ops, mirror, two, [0, 0, 8, 8, 16, 16], 7, "hand-built with empty segments", weighted=weighted, fill_value=2.0)
    check_call(ops, mirror, two, [0, 8, 16], 7, "hand-built, weights as they are", weighted=weighted, normalize=False)


# ------------------------------------------------------------------------------------------------ 4. transpose identity, autograd
def fsum_dot(a, b):
    """The sum of the rounded products, exactly: one rounding per product."""
    return math.fsum((a.detach().cpu().double() * b.detach().cpu().double()).reshape(-1).tolist())


@pytest.mark.parametrize("o_v", ["random", "degree"])
def test_transpose_identity(ops, o_v):
    """<P x, z> == <x, P^T z>: each side within its own bound of item 1 (weighted by the other factor), the dot products within one
    rounding per product (math.fsum adds them exactly)."""
    n, F = 3000, 16
    sc, ptr = depths_views(ops, n, 5, 2, o_v, [n // 8, n // 4, n // 2])
    x, z = features(n, F, 6, seed=1), features(n, F, 6, seed=2)
    y = ops.snapshot_propagate(sc, ptr, n, x.cuda(), weighted=True)
    yt = ops.snapshot_propagate(sc, ptr, n, z.cuda(), weighted=True, transpose=True)
    _, A, _, longest = yardstick(sc, ptr, n, x, weighted=True)
    _, At, _, longest_t = yardstick(sc, ptr, n, z, transpose=True, weighted=True)
    factor = bound_factor(max(longest, longest_t), True)
    tol = factor * (float((A * z.abs()).sum()) + float((At * x.abs()).sum())) * (1 + 1e-9)
    tol += U * (float((y.cpu().abs() * z.abs()).sum()) + float((yt.cpu().abs() * x.abs()).sum()))
    lhs, rhs = fsum_dot(y, z), fsum_dot(x, yt)
    print(f"{o_v}: <Px, z> - <x, P^T z> = {lhs - rhs:.3e} (bound {tol:.3e}), <Px, z> = {lhs:.6e}")
    assert abs(lhs - rhs) <= tol


def dense_layers(sc, ptr, n, **kw):
    """A^_l as dense float64 matrices [target, source] from the yardstick's entries, and sum |entries| for the bounds."""
    segs = segments(ptr, n, None)
    mats = torch.zeros(len(segs), n, n, dtype=torch.float64)
    longest = 0
    for s, l, lo, hi, r0, r1 in segs:
        src, dst, val = torch_segment(sc[r0:r1], lo, hi, **flags_of(kw))
        assert torch.unique(dst * n + src).numel() == src.numel(), "no pair twice: index_put_ adds nothing up"
        mats[l].index_put_((dst, src), val, accumulate=True)
        longest = max(longest, int(torch.bincount(dst).max()) - 1, int(torch.bincount(src).max()) - 1)
    return mats, longest


@pytest.mark.parametrize("per_layer", [False, True])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gradient_against_the_dense_matrix(ops, per_layer, dtype):
    n, F = 500, 16
    sc, ptr = depths_views(ops, n, 3, 5, "random", [n // 4, n // 2])
    L = ptr.numel() - 1
    mats, longest = dense_layers(sc, ptr, n, weighted=True)
    x64 = features(n, F, L if per_layer else None, seed=3).to(dtype).double()
    z64 = features(n, F, L, seed=4).to(dtype).double()
    x = x64.to(dtype).cuda().requires_grad_(True)
    y = ops.snapshot_propagate(sc, ptr, n, x, weighted=True)
    assert y.requires_grad and y.dtype == dtype
    (y * z64.to(dtype).cuda()).sum().backward()
    assert ops.last_stats["host_syncs"] == HOST_SYNCS
    g_layers = torch.einsum("lts,ltf->lsf", mats, z64)                       # A^_l^T z_l
    A_layers = torch.einsum("lts,ltf->lsf", mats.abs(), z64.abs())
    ref, A = (g_layers, A_layers) if per_layer else (g_layers.sum(0), A_layers.sum(0))
    factor = bound_factor(longest, True) + (0 if per_layer else (L - 1) * U)   # (the sum over the layers)
    if dtype == torch.float32:
        factor += 2.0 ** -24 * (1 if per_layer else 2 * L)                     # every layer's result rounded once, and their float32 sum
    err = (x.grad.detach().cpu().double() - ref).abs()
    worst = float((err / A.clamp_min(1e-300)).max())
    print(f"gradient per_layer={per_layer} {dtype}: max error / A = {worst:.3e} (bound {factor:.3e})")
    assert x.grad.shape == x.shape and x.grad.dtype == dtype and bool((err <= factor * A).all())
    assert sc.grad is None


def test_gradcheck_and_no_double_backward(ops):
    n = 40
    sc, ptr = depths_views(ops, n, 2, 7, "random", [n // 4, n // 2])
    for layers, kw in ((None, {}), (4, {}), (None, {"transpose": True}), (4, {"weighted": True, "fill_value": 2.0})):
        x = torch.randn((n, 3) if layers is None else (layers, n, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(5))
        x = x.cuda().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda t: ops.snapshot_propagate(sc, ptr, n, t, **kw), (x,), eps=1e-6, atol=1e-7, rtol=1e-7)
    x = features(n, 3).cuda().requires_grad_(True)
    (g,) = torch.autograd.grad(ops.snapshot_propagate(sc, ptr, n, x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    with torch.no_grad():
        assert not ops.snapshot_propagate(sc, ptr, n, x).requires_grad


# ------------------------------------------------------------------------------------------------ 5. the adapters
@pytest.mark.parametrize("which", ["rLap", "rLapViews", "rLapDepths"])
def test_snapshots_describe_the_rows_of_augment(ops, which):
    from rlap_amd.adapters import Graph, Snapshots, rLap, rLapDepths, rLapViews
    n = 1200
    x = torch.randn(n + 50, 8, generator=torch.Generator().manual_seed(0)).cuda()     # more rows than max id + 1
    g = Graph(x, torch.from_numpy(ba_graph(n, 4, 3)).cuda(), None)
    make = {"rLap": lambda: rLap(0.3, "random", "asc", keep_weights=True, seed=8),
            "rLapViews": lambda: rLapViews((0.3, 0.45), "random", "asc", keep_weights=True, seed=8),
            "rLapDepths": lambda: rLapDepths((0.1, 0.3, 0.5), "random", "asc", keep_weights=True, seed=8, views=2)}[which]
    graphs = make().augment(g)
    if which == "rLap":
        graphs = [graphs]
    if which == "rLapDepths":                                                # R lists of K -> depth-major, then view
        graphs = [graphs[r][k] for k in range(3) for r in range(2)]
    snaps = make().snapshots(g)
    assert isinstance(snaps, Snapshots) and snaps.num_nodes == n + 50 and snaps.weighted and snaps.node_ptr is None
    p = torch.as_tensor(snaps.ptr).tolist()
    assert snaps.layers == len(graphs) == len(p) - 1
    for k, gr in enumerate(graphs):
        part = snaps.sc[p[k]:p[k + 1]]
        assert torch.equal(part[:, :2].long().t(), gr.edge_index) and same_bits(part[:, 2], gr.edge_weights), f"{which} view {k}"
    y = snaps.propagate(x)
    assert y.shape == (len(graphs), n + 50, 8) and y.dtype == torch.float32
    assert same_bits(y, ops.snapshot_propagate(snaps.sc, snaps.ptr, n + 50, x, weighted=True))
    assert same_bits(snaps.propagate(x, transpose=True), ops.snapshot_propagate(snaps.sc, snaps.ptr, n + 50, x, weighted=True, transpose=True))
    assert not type(make())(0.3 if which == "rLap" else (0.3,), keep_weights=False, seed=8).snapshots(g).weighted


def test_snapshot_gcn_conv_against_the_dense_product(ops):
    """Output and the gradients of W, b and x against D^-1/2 (A + I) D^-1/2 @ (x @ W) + b per view, A[target, source] += w from
    .augment(g) of the same seed.  Bounds: the sparse product's (16 + 4 L) u of item 1, plus 2 K u for a dense product of inner
    dimension K on each side (K = in_channels for x @ W, out_channels for the gradient of x, n for the gradient of W; 2 n layers
    for the bias), each times the sum of the absolute values of the terms."""
    from rlap_amd.adapters import Graph, SnapshotGCNConv, rLapViews
    n, cin, cout = 500, 8, 5
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    aug = lambda: rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2)
    views, snaps = aug().augment(g), aug().snapshots(g)
    mats, longest = [], 0
    for v in views:
        A = torch.zeros(n, n, dtype=torch.float64)
        A.index_put_((v.edge_index[1].cpu(), v.edge_index[0].cpu()), v.edge_weights.cpu(), accumulate=True)
        longest = max(longest, int((A != 0).sum(1).max()), int((A != 0).sum(0).max()))
        A = A + torch.eye(n, dtype=torch.float64)
        dis = A.sum(1).pow(-0.5)
        mats.append(dis[:, None] * A * dis[None, :])
    mats = torch.stack(mats)
    torch.manual_seed(3)
    conv = SnapshotGCNConv(cin, cout).double().cuda()
    with torch.no_grad():
        conv.bias.copy_(torch.randn(cout))
    x = features(n, cin, seed=6).cuda().requires_grad_(True)
    z = features(n, cout, 2, seed=7)
    out = conv(x, snaps)
    assert out.shape == (2, n, cout) and out.dtype == torch.float64
    (out * z.cuda()).sum().backward()
    W, b, xr = (t.detach().cpu().clone().requires_grad_(True) for t in (conv.weight, conv.bias, x))
    ref = mats @ (xr @ W) + b
    (ref * z).sum().backward()
    sp = bound_factor(longest, True)
    aW, ax, am, az = W.detach().abs(), xr.detach().abs(), mats.abs(), z.abs()
    atz = torch.einsum("lts,ltf->sf", am, az)                                # sum over the views of |A^|^T |z|
    checks = [("output", out, ref.detach(), (sp + 2 * cin * U) * (am @ (ax @ aW)) + 2 * U * b.detach().abs()),
              ("grad W", conv.weight.grad, W.grad, (sp + 2 * (n + 2) * U) * (ax.t() @ atz)),
              ("grad b", conv.bias.grad, b.grad, 2 * (2 * n) * U * az.sum((0, 1))),
              ("grad x", x.grad, xr.grad, (sp + 2 * (cout + 2) * U) * (atz @ aW.t()))]
    for what, got, want, tol in checks:
        err = (got.detach().cpu() - want).abs()
        print(f"SnapshotGCNConv {what}: max error {float(err.max()):.3e}, max error / bound {float((err / tol.clamp_min(1e-300)).max()):.3e}")
        assert got.shape == want.shape and bool((err <= tol).all()), what
    out3 = conv(torch.stack([x.detach(), x.detach()]), snaps)                # per-layer features: the later layers
    assert out3.shape == out.shape and torch.allclose(out3, out, rtol=1e-12, atol=0)


# ------------------------------------------------------------------------------------------------ 6. info and errors
def test_errors_leave_the_handle_intact(ops, mirror):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    x = features(n, 16).cuda()
    p = ptr.tolist()
    shuffled = sc.clone()
    perm = torch.randperm(p[1], generator=torch.Generator().manual_seed(0)).cuda()
    shuffled[:p[1]] = sc[:p[1]][perm]
    bad = sc.clone()
    bad[5, 0] = n + 3
    for transpose in (False, True):
        with pytest.raises(ValueError, match="contiguous|grouped"):
            ops.snapshot_propagate(shuffled, ptr, n, x, transpose=transpose)
        with pytest.raises(ValueError, match="range"):
            ops.snapshot_propagate(bad, ptr, n, x, transpose=transpose)
    lonely = torch.tensor([[0, 1, 1.0], [2, 1, 1.0], [1, 0, 1.0]], dtype=torch.float64).cuda()   # source 2 has no column block
    for transpose in (False, True):
        with pytest.raises(ValueError, match="symmetric"):
            ops.snapshot_propagate(lonely, [0, 3], 3, features(3, 3).cuda(), transpose=transpose)
    two = torch.tensor([[0, 1, 1.0], [1, 0, 1.0], [3, 4, 1.0], [4, 3, 1.0]], dtype=torch.float64).cuda()
    x6 = features(6, 3).cuda()
    ok = ops.snapshot_propagate(two, [0, 2, 4], 6, x6, node_ptr=[0, 3, 6])
    assert ok.shape == (1, 6, 3) and ops.last_stats["host_syncs"] == HOST_SYNCS
    with pytest.raises(ValueError, match="range"):
        ops.snapshot_propagate(two, [0, 1, 4], 6, x6, node_ptr=[0, 3, 6])       # row (1, 0) in graph 1
    for w in (0.0, -1.0, float("nan"), float("inf")):
        bad = sc.clone()
        bad[7, 2] = w
        with pytest.raises(ValueError):
            ops.snapshot_propagate(bad, ptr, n, x, weighted=True)
        ops.snapshot_propagate(bad, ptr, n, x)                                  # unweighted: the weights are not looked at
    check_call(ops, mirror, sc, ptr, n, "after the errors", Fs=(16,), weighted=True)
