"""Edge plans on the device: ops.edge_list_plan / ops.edge_plan, adapters.graph_plan, rLapDepths.diffuse_plan.

Two yardsticks, neither of them the code under test:
  * bits -- on an input in the elimination layout the plan equals ops.snapshot_plan's and its products equal that plan's by
    torch.equal; on any other input the decoded buffer equals the host mirror (tests/csrc/edgeplan_mirror.cc around the headers the
    kernels include), whose degree rule tests/test_edge_plan_cpu.py ties to numpy;
  * the float64 torch formulation of tests/test_gpu_propagate.py (index_add_, or the dense matrix), within its derived bound
    (16 + 4 L) 2^-53 A, L the longest list of the call plus one.
"""
import numpy as np
import pytest
import torch

import edgeplan_mirror
import plan_buffer
import spmm_mirror
from test_gpu_propagate import U, assert_close, bound_factor, dense_layers, yardstick
from util import ba_graph

pytestmark = pytest.mark.gpu

LIST_KW = [dict(weighted=w, add_self_loops=l, normalize=nz) for w in (False, True) for l in (True, False) for nz in (True, False)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mirrors(tmp_path_factory):
    d = tmp_path_factory.mktemp("edgeplan")
    return edgeplan_mirror.build(d), spmm_mirror.build(d)


@pytest.fixture(scope="module")
def elim(ops):
    """BA(300, 3), three depths x two views, per order: computed once, never changed."""
    n = 300
    ei = torch.from_numpy(ba_graph(n, 3, 2)).cuda()
    out = {}
    for o_v in ("random", "degree", "coarsen"):
        sc, ptr = ops.approximate_cholesky_depths(ei, None, n, [n // 8, n // 4, n // 2], o_v, "asc", views=2, seed=11, return_device="same")
        assert ptr.numel() == 7
        out[o_v] = (sc, ptr.tolist(), n)
    return out


def decode(plan):
    return plan_buffer.decode(plan.buffer.cpu().numpy(), plan.desc)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_parts(got, want, what):
    """Two decoded plans part by part: a failure names the part."""
    assert got["slots"] == want["slots"], what
    assert (got["loopc"] is None) == (want["loopc"] is None), f"{what}: loopc[] present"
    if got["loopc"] is not None:
        assert np.array_equal(bits(got["loopc"]), bits(want["loopc"])), f"{what}: loopc[]"
    for name, _ in plan_buffer.DIRECTIONS:
        a, b = got[name], want[name]
        assert (a is None) == (b is None), f"{what}: {name} built"
        if a is None:
            continue
        assert np.array_equal(a["off"], b["off"]), f"{what} {name}: off[]"
        assert (a["entries"], a["chunks"]) == (b["entries"], b["chunks"]), f"{what} {name}: entries / chunks"
        assert np.array_equal(a["dir_slot"], b["dir_slot"]) and np.array_equal(a["dir_k"], b["dir_k"]), f"{what} {name}: the directory"
        assert np.array_equal(a["id"], b["id"]), f"{what} {name}: record ids"
        assert np.array_equal(bits(a["c"]), bits(b["c"])), f"{what} {name}: coefficient bits"
        assert not a["zero"].any() and not b["zero"].any(), f"{what} {name}: zero words"
    assert plan_buffer.same_decoded(got, want), what


def shuffled(sc, ptr, seed):
    g = torch.Generator().manual_seed(seed)
    out = sc.clone()
    for s in range(len(ptr) - 1):
        if ptr[s + 1] > ptr[s]:
            out[ptr[s]:ptr[s + 1]] = sc[ptr[s]:ptr[s + 1]][torch.randperm(ptr[s + 1] - ptr[s], generator=g).to(sc.device)]
    return out


def against_mirror(ops, ep, rows, ptr, n, what, node_ptr=None, directions="both", **kw):
    """One device build against the host mirror, bit for bit; the descriptor and the report.  Returns (plan, decoded)."""
    plan = ops.edge_list_plan(rows, ptr, n, node_ptr=node_ptr, directions=directions, **kw)
    info = dict(ops.last_stats)
    assert info["host_syncs"] == 1, what
    dec = decode(plan)
    host = rows.detach().cpu().double().numpy()
    want = edgeplan_mirror.plan(ep, host, ptr, n, node_ptr=node_ptr, directions=directions, **kw)
    same_parts(dec, want, what)
    loops = kw.get("add_self_loops", True)
    assert info["loops_removed"] == want["loops_removed"] and plan.entries == host.shape[0] + (dec["slots"] - want["loops_removed"] if loops else 0), what
    G = len(node_ptr) - 1 if node_ptr is not None else 1
    lists = plan_buffer.expected_lists(host, ptr, n, G, False, False)
    assert info["blocks"] == len(lists), f"{what}: blocks is the number of non-empty forward lists"
    assert int(plan.desc.plan_bytes) == plan.nbytes and int(plan.desc.magic) == 0x504C414E and int(plan.desc.m) == host.shape[0]
    for name, lo, hi in dec["spans"]:
        assert 0 <= lo <= hi <= plan.nbytes, (what, name)
    return plan, dec


def product_close(plan, rows, ptr, n, what, node_ptr=None, F=3, **kw):
    """plan.propagate against the float64 index_add_ reference, both directions, within the derived bound."""
    x = torch.randn(n, F, dtype=torch.float64, generator=torch.Generator().manual_seed(F))
    for transpose in (False, True):
        y = plan.propagate(x.cuda(), transpose=transpose)
        ref, A, count, longest = yardstick(rows, ptr, n, x, node_ptr=node_ptr, transpose=transpose, **kw)
        assert_close(y, ref, A, count, bound_factor(longest, True), f"{what} {'T' if transpose else 'N'}")


def features(n, F, layers, dtype, seed=0):
    shape = (n, F) if layers is None else (layers, n, F)
    g = torch.Generator().manual_seed(1000 * F + seed + (7 if layers else 0))
    x = torch.randn(shape, dtype=torch.float64, generator=g) * (10.0 ** torch.randint(-2, 3, shape, generator=g).double())
    return x.to(dtype).cuda()


# ------------------------------------------------------------------------------------------------ 1. the elimination layout: same bits
@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_same_bits_as_snapshot_plan_on_the_elimination_layout(ops, elim, o_v):
    sc, ptr, n = elim[o_v]
    L = len(ptr) - 1
    for kw in LIST_KW:
        for directions in ("both", "forward", "transposed"):
            tag = f"{o_v} {kw} {directions}"
            want = ops.snapshot_plan(sc, ptr, n, directions=directions, **kw)
            got = ops.edge_list_plan(sc, ptr, n, directions=directions, **kw)
            same_parts(decode(got), decode(want), tag)
            assert int(got.desc.plan_bytes) == int(want.desc.plan_bytes) and got.nbytes == want.nbytes, f"{tag}: plan_bytes"
            assert got.entries == want.entries and got.info["loops_removed"] == want.info["loops_removed"] == 0
            assert got.info["blocks"] == want.info["blocks"], tag
            for F in (3, 64):
                for dtype in (torch.float32, torch.float64):
                    for per_layer in (False, True):
                        x = features(n, F, L if per_layer else None, dtype)
                        for transpose in (False, True):
                            if directions != "both" and (directions == "transposed") != transpose:
                                continue
                            y, ref = got.propagate(x, transpose=transpose), want.propagate(x, transpose=transpose)
                            assert y.dtype == ref.dtype and torch.equal(y, ref), f"{tag} F={F} {dtype} per_layer={per_layer} T={transpose}"


# ------------------------------------------------------------------------------------------------ 2. any order
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_rows_in_any_order(ops, mirrors, elim, o_v, weighted):
    ep, _ = mirrors
    sc, ptr, n = elim[o_v]
    rows = shuffled(sc, ptr, 5)
    assert not torch.equal(rows, sc)
    tag = f"{o_v} shuffled weighted={weighted}"
    plan, dec = against_mirror(ops, ep, rows, ptr, n, tag, weighted=weighted)
    product_close(plan, rows, ptr, n, tag, weighted=weighted)
    again = ops.edge_list_plan(rows, ptr, n, weighted=weighted)
    assert plan_buffer.same_decoded(decode(again), dec), f"{tag}: two builds differ"
    for poison in (0xFF, 0x00):
        try:
            ops.debug_set_poison(poison)
            other = ops.edge_list_plan(rows, ptr, n, weighted=weighted)
        finally:
            ops.debug_set_poison(-1)
        assert plan_buffer.same_decoded(decode(other), dec), f"{tag}: the content depends on what the buffer and the arena held ({poison:#x})"
    against_mirror(ops, ep, rows, ptr, n, tag + " no loops", weighted=weighted, add_self_loops=False)
    against_mirror(ops, ep, rows, ptr, n, tag + " plain weights", weighted=weighted, normalize=False, fill_value=2.0)


# ------------------------------------------------------------------------------------------------ 3. the lanes of the degree rule
DEGREES = (0, 1, 15, 16, 17, 63, 64, 65, 129)


def comb(seed):
    """Layer 0: targets 0..8 with in-degrees DEGREES from sources 9..; layer 1: the same rows turned round, so ids 0..8 have those
    out-degrees.  Two or three loop rows on some of them.  Shuffled per segment."""
    rs = np.random.RandomState(seed)
    a = []
    for j, d in enumerate(DEGREES):
        a += [[9 + k, j, 0.25 + rs.rand() * 10.0 ** rs.randint(-3, 4)] for k in range(d)]
        a += [[j, j, 0.5 + rs.rand()] for _ in range(j % 4)]
    a = np.array(a, dtype=np.float64)
    b = a[:, [1, 0, 2]].copy()
    rs.shuffle(a)
    rs.shuffle(b)
    return torch.from_numpy(np.concatenate([a, b])).cuda(), [0, len(a), 2 * len(a)], 9 + max(DEGREES)


@pytest.mark.parametrize("weighted", [False, True])
def test_comb_of_the_lane_boundaries(ops, mirrors, weighted):
    ep, _ = mirrors
    rows, ptr, n = comb(3)
    for loops in (True, False):
        tag = f"comb weighted={weighted} loops={loops}"
        plan, dec = against_mirror(ops, ep, rows, ptr, n, tag, weighted=weighted, add_self_loops=loops)
        got = np.diff(dec["forward"]["off"])[:9].tolist()
        assert got == [d + (0 if loops else j % 4) for j, d in enumerate(DEGREES)], tag
        assert np.diff(dec["transposed"]["off"])[n:n + 9].tolist() == got, tag
    product_close(plan, rows, ptr, n, tag, weighted=weighted, add_self_loops=False)


# ------------------------------------------------------------------------------------------------ 4. chunks
@pytest.mark.parametrize("leaves,chunks", [(256, 0), (257, 2), (515, 3)])
def test_stars_of_one_two_and_three_chunks(ops, mirrors, leaves, chunks):
    ep, _ = mirrors
    rs = np.random.RandomState(leaves)
    w = rs.rand(leaves) + 0.5
    rows = np.array([[i + 1, 0, w[i]] for i in range(leaves)] + [[0, i + 1, w[i] * (1.0 + 2.0 ** -50 * (i % 3))] for i in range(leaves)])
    rs.shuffle(rows)
    rows, ptr, n = torch.from_numpy(rows).cuda(), [0, 2 * leaves], leaves + 1
    tag = f"star of {leaves} leaves"
    plan, dec = against_mirror(ops, ep, rows, ptr, n, tag, weighted=True)
    assert plan.desc.chunks_forward == chunks == plan.desc.chunks_transposed and plan.info["chunked_lists_forward"] == (1 if chunks else 0)
    x = features(n, 5, None, torch.float64)
    ys = [plan.propagate(x, transpose=t) for t in (False, True)]
    try:
        ops.debug_set_limits(scratch_entries=0)                               # no chunk sum kept: one group sums the list, same bits
        for t in (False, True):
            assert torch.equal(plan.propagate(x, transpose=t), ys[t]), f"{tag}: scratch_entries=0 T={t}"
    finally:
        ops.debug_set_limits(scratch_entries=-1)
    product_close(plan, rows, ptr, n, tag, weighted=True)
    for directions in ("forward", "transposed"):
        against_mirror(ops, ep, rows, ptr, n, f"{tag} {directions}", directions=directions, weighted=True)


# ------------------------------------------------------------------------------------------------ 5. a hand-made directed list
# num_nodes 9, six ids used: duplicate rows, three loop rows on id 2 with different weights (the last one's is the loop's), id 5 only
# a source, id 6 only a target, ids 4, 7 and 8 absent
HAND_A = [[0, 1, 0.5], [2, 2, 3.0], [1, 0, 0.25], [0, 1, 0.5], [5, 0, 1.5], [2, 2, 4.0], [3, 6, 2.0], [1, 2, 0.75], [2, 2, 5.0], [2, 1, 1.25],
          [0, 3, 0.125]]
HAND_B = [[3, 0, 1.0], [0, 3, 2.0], [5, 6, 0.5], [1, 1, 9.0]]


@pytest.mark.parametrize("weighted", [False, True])
def test_hand_made_directed_list(ops, mirrors, weighted):
    ep, _ = mirrors
    rows = torch.tensor(HAND_A + HAND_B, dtype=torch.float64).cuda()
    ptr, n = [0, 11, 11, 15], 9                                               # an empty segment between the two
    for kw in (dict(), dict(fill_value=2.0), dict(add_self_loops=False), dict(normalize=False), dict(add_self_loops=False, normalize=False)):
        tag = f"hand-made weighted={weighted} {kw}"
        plan, dec = against_mirror(ops, ep, rows, ptr, n, tag, weighted=weighted, **kw)
        assert ops.last_stats["host_syncs"] == 1 and plan.layers == 3
        product_close(plan, rows, ptr, n, tag, weighted=weighted, **kw)
        if kw.get("add_self_loops", True):
            assert plan.info["loops_removed"] == 4
            if kw.get("normalize", True) is False:
                assert dec["loopc"][2] == (5.0 if weighted else 1.0) and dec["loopc"][4] == kw.get("fill_value", 1.0)   # the last loop row's weight
            if "fill_value" not in kw:
                assert bool((dec["loopc"][n:2 * n] == 1.0).all())             # the empty segment: unit loops alone
    # the dense reference, loops on: D^-1/2 (A + loops) D^-1/2 with A[target, source] += w
    x = torch.randn(n, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    plan = ops.edge_list_plan(rows, ptr, n, weighted=True)
    host = rows.cpu()
    for layer, (r0, r1) in enumerate(((0, 11), (11, 11), (11, 15))):
        M, lw = torch.zeros(n, n, dtype=torch.float64), torch.ones(n, dtype=torch.float64)
        for i, j, w in host[r0:r1].tolist():
            if i == j:
                lw[int(i)] = w
            else:
                M[int(j), int(i)] += w
        M = M + torch.diag(lw)
        dis = M.sum(1).pow(-0.5)
        Ah = dis[:, None] * M * dis[None, :]
        for transpose in (False, True):
            y = plan.propagate(x.cuda(), transpose=transpose)[layer].cpu()
            mat = Ah.t() if transpose else Ah
            tol = bound_factor(3, True) * (mat.abs() @ x.abs())                   # (three rows is the longest list, by target 1 and by source 0)
            assert bool(((y - mat @ x).abs() <= tol).all()), f"dense, layer {layer} T={transpose}"
    empty = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    plan, dec = against_mirror(ops, ep, empty, [0, 0, 0], 5, "m = 0", weighted=weighted)
    assert plan.entries == 10 and ops.last_stats["blocks"] == 0
    assert torch.equal(plan.propagate(x[:5].cuda()), x[:5].cuda().expand(2, 5, 4))
    plan, _ = against_mirror(ops, ep, empty, [0, 0], 5, "m = 0 without loops", add_self_loops=False)
    assert bool((plan.propagate(x[:5].cuda()) == 0).all())


# ------------------------------------------------------------------------------------------------ 6. a batch
def test_node_ptr_batch_of_three_graphs(ops, mirrors):
    ep, _ = mirrors
    sizes = [40, 1, 60]
    node_ptr = [0, 40, 41, 101]
    rs = np.random.RandomState(2)
    parts, ptr = [], [0]
    for layer in range(2):
        for g, (k, m) in enumerate(((40, 2), (1, 0), (60, 3))):
            if k >= 4:
                ei = ba_graph(k, m, 10 * layer + g) + node_ptr[g]
                part = np.stack([ei[0], ei[1], rs.rand(ei.shape[1]) + 0.5], 1).astype(np.float64)
                if layer == 1:
                    part = part[: part.shape[0] // 2]                          # directed: half of the rows only
                rs.shuffle(part)
                parts.append(part)
            ptr.append(ptr[-1] + (len(parts[-1]) if k >= 4 else 0))
    rows = torch.from_numpy(np.concatenate(parts)).cuda()
    n = sum(sizes)
    for weighted in (False, True):
        plan, dec = against_mirror(ops, ep, rows, ptr, n, f"batch weighted={weighted}", node_ptr=node_ptr, weighted=weighted)
        assert plan.layers == 2
        product_close(plan, rows, ptr, n, f"batch weighted={weighted}", node_ptr=node_ptr, weighted=weighted)
    bad = rows.clone()
    bad[ptr[2], 0] = 3.0                                                      # an id of graph 0 inside graph 2's segment
    with pytest.raises(ValueError, match="an id of the rows"):
        ops.edge_list_plan(bad, ptr, n, node_ptr=node_ptr)
    assert ops.edge_list_plan(bad, ptr, n).layers == 6                        # (without node_ptr the id is in range)


# ------------------------------------------------------------------------------------------------ 7. PPR
def test_ppr_diffused_snapshots(ops, mirrors):
    from rlap_amd.adapters import Graph, rLapDepths
    ep, _ = mirrors
    n = 200
    ei = torch.from_numpy(ba_graph(n, 3, 4)).cuda()
    aug = lambda: rLapDepths((1 / 8, 1 / 4), "random", "asc", seed=6)
    g = Graph(None, ei, None)
    _, sc, ptr, nn = aug()._snapshots(g)
    assert nn == n and ptr.tolist()[-1] == sc.shape[0]
    out, pptr = ops.snapshot_ppr(sc, ptr, n)
    pp = pptr.tolist()
    assert len(pp) == 3 and out.shape[0] == pp[-1] > 0
    with pytest.raises(ValueError):
        ops.snapshot_plan(out, pp, n, weighted=True)                          # grouped by row id: not the elimination layout
    plan, dec = against_mirror(ops, ep, out, pp, n, "ppr", weighted=True)
    mats, longest = dense_layers(out, pp, n, weighted=True)                   # D^-1/2 (S + I) D^-1/2, [target, source]
    x = torch.randn(n, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    for transpose in (False, True):
        m_ = mats.transpose(1, 2) if transpose else mats
        y = plan.propagate(x.cuda(), transpose=transpose).cpu()
        err, A = (y - m_ @ x).abs(), m_.abs() @ x.abs()
        print(f"ppr T={transpose}: max error / A = {float((err / A.clamp_min(1e-300)).max()):.3e} (bound {bound_factor(longest, True):.3e})")
        assert bool((err <= bound_factor(longest, True) * A).all()), f"ppr T={transpose}"
    other = aug().diffuse_plan(g)
    assert other.layers == 2 and other.num_nodes == n and plan_buffer.same_decoded(decode(other), dec), "diffuse_plan: another buffer"
    assert desc_equal(other.desc, plan.desc)


def desc_equal(a, b):
    return all(getattr(a, f) == getattr(b, f) for f, _ in a._fields_)


# ------------------------------------------------------------------------------------------------ 8. the encoder
def test_grace_shaped_step(ops):
    """One SnapshotGCNConv stack on graph_plan(g) (z) and on the two views' plan (z1, z2).  z against the dense float64
    A^ (X W) + b, A^ = D^-1/2 (A + I) D^-1/2; the gradients of W, b and x against the dense matrix, with the bounds of
    tests/test_gpu_propagate.py::test_snapshot_gcn_conv_against_the_dense_product."""
    from rlap_amd.adapters import Graph, SnapshotGCNConv, graph_plan, rLapViews
    n, cin, cout = 300, 8, 5
    ei = torch.from_numpy(ba_graph(n, 3, 5)).cuda()
    xg = torch.randn(n, cin, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    g = Graph(xg.cuda(), ei, None)
    plan = graph_plan(g)
    assert isinstance(plan, ops.SnapshotPlan) and plan.layers == 1 and plan.num_nodes == n and plan.entries == ei.shape[1] + n
    views = rLapViews((0.25, 0.4), "random", "asc", seed=2).snapshots(g).plan()
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((ei[1].cpu(), ei[0].cpu()), torch.ones(ei.shape[1], dtype=torch.float64), accumulate=True)
    longest = int((A != 0).sum(1).max())
    A = A + torch.eye(n, dtype=torch.float64)
    dis = A.sum(1).pow(-0.5)
    mat = dis[:, None] * A * dis[None, :]
    torch.manual_seed(3)
    conv = SnapshotGCNConv(cin, cout).double().cuda()
    with torch.no_grad():
        conv.bias.copy_(torch.randn(cout))
    x = xg.cuda().requires_grad_(True)
    zc = torch.randn(n, cout, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    z = conv(x, plan)
    z12 = conv(x, views)
    assert z.shape == (1, n, cout) and z12.shape == (2, n, cout) and z.dtype == torch.float64
    loss = (z[0] * zc.cuda()).sum() + 0.0 * z12.sum()                       # (the views' branch reaches W, b and x too; its weight is 0)
    loss.backward()
    W, b, xr = (t.detach().cpu().clone().requires_grad_(True) for t in (conv.weight, conv.bias, x))
    ref = mat @ (xr @ W) + b
    (ref * zc).sum().backward()
    sp = bound_factor(longest, True)
    aW, ax, am, az = W.detach().abs(), xr.detach().abs(), mat.abs(), zc.abs()
    atz = am.t() @ az
    checks = [("z", z[0], ref.detach(), (sp + 2 * cin * U) * (am @ (ax @ aW)) + 2 * U * b.detach().abs()),
              ("grad W", conv.weight.grad, W.grad, (sp + 2 * (n + 2) * U) * (ax.t() @ atz)),
              ("grad b", conv.bias.grad, b.grad, 2 * n * U * az.sum(0)),
              ("grad x", x.grad, xr.grad, (sp + 2 * (cout + 2) * U) * (atz @ aW.t()))]
    for what, got, want, tol in checks:
        err = (got.detach().cpu() - want).abs()
        print(f"encoder {what}: max error {float(err.max()):.3e}, max error / bound {float((err / tol.clamp_min(1e-300)).max()):.3e}")
        assert got.shape == want.shape and bool((err <= tol).all()), what
    # a real step: both branches with weight, every parameter reached
    conv.zero_grad()
    x.grad = None
    (conv(x, plan).sum() + conv(x, views).pow(2).sum()).backward()
    assert all(t.grad is not None and bool(t.grad.abs().sum() > 0) for t in (conv.weight, conv.bias, x))
    one = graph_plan(g, directions="forward")
    with pytest.raises(ValueError, match="forward"):
        conv(x, one)                                                          # x @ W requires a gradient: the backward needs the other direction
    with torch.no_grad():
        assert torch.equal(conv(x, one), conv(x, plan))


# ------------------------------------------------------------------------------------------------ 9. errors
def test_errors_raise_value_error_and_leave_the_handle_intact(ops, mirrors):
    ep, _ = mirrors
    good = torch.tensor(HAND_A, dtype=torch.float64).cuda()
    n = 9

    def altered(r, c, v):
        t = good.clone()
        t[r, c] = v
        return t
    for what, rows, kw, msg in [("id 1.5", altered(3, 0, 1.5), {}, "an id of the rows"), ("id -1", altered(4, 1, -1.0), {}, "an id of the rows"),
                                ("id num_nodes", altered(0, 1, float(n)), {}, "an id of the rows"),
                                ("id NaN", altered(0, 0, float("nan")), {}, "an id of the rows"),
                                ("NaN weight", altered(2, 2, float("nan")), dict(weighted=True), "a weight is not finite"),
                                ("weight 0", altered(6, 2, 0.0), dict(weighted=True), "a weight is not finite"),
                                ("weight inf", altered(6, 2, float("inf")), dict(weighted=True), "a weight is not finite")]:
        with pytest.raises(ValueError, match=msg):
            ops.edge_list_plan(rows, [0, 11], n, **kw)
    ops.edge_list_plan(altered(6, 2, 0.0), [0, 11], n, weighted=True, normalize=False)        # (a weight is checked only when it is divided by)
    ops.edge_list_plan(altered(6, 2, 0.0), [0, 11], n)
    with pytest.raises(ValueError, match="ptr"):
        ops.edge_list_plan(good, [0, 12], n)                                                  # a malformed ptr: before the device
    against_mirror(ops, ep, good, [0, 11], n, "after the errors", weighted=True)
    ei = good[:, :2].long().t().contiguous()
    with pytest.raises(ValueError, match="an id of the rows"):
        ops.edge_plan(ei, None, 3)
    plan = ops.edge_plan(ei, good[:, 2])
    assert plan.num_nodes == 7 and plan_buffer.same_decoded(decode(plan), decode(ops.edge_list_plan(good, [0, 11], 7, weighted=True)))
