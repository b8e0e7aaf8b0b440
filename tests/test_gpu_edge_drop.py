"""Edge dropping on the device: ops.drop_edges and the adapters on it, against the host mirror
(tests/csrc/edgedrop_mirror.cc around rlap_amd/csrc/rlap_edgedrop.h, the header the kernels include), whose rules
tests/test_edge_drop_cpu.py ties to numpy on the very inputs used here (tests/edge_drop_cases.py).

  * centrality: bit for bit, all three schemes, every graph -- the operations are IEEE add, multiply, divide and square root;
  * node_weight: through the device's float64 log, which may differ from the host's in the last place; smax - s cancels, so the
    bound is absolute: |difference| <= 8 * 2^-52 * max|s| / (smax - smean);
  * the mask: equal outside the band |u - q| <= 1e-9, which the CPU suite shows to be empty for these cases;
  * rows / ptr: the input rows at the mask's positions, in order, view-major.

Measured on an MI355X: the largest node_weight difference is 8.9e-16 (the directed list, pagerank, bound 5.6e-15), 0 in 14 of the 18
scored cases that are not the ring."""
import numpy as np
import pytest
import torch

import edge_drop_cases as cases
import edgedrop_mirror

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return edgedrop_mirror.build(tmp_path_factory.mktemp("edgedrop"))


def device_graph(name):
    src, dst, n = cases.graph(name)
    return src, dst, n, torch.from_numpy(np.stack([src, dst])).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def expected_rows(src, dst, w, mask):
    parts = [np.stack([src[m], dst[m], (w[m] if w is not None else np.ones(int(m.sum())))], 1) for m in mask]
    return np.concatenate(parts).reshape(-1, 3), [0] + np.cumsum(mask.sum(1)).tolist()


@pytest.mark.parametrize("name,scheme,aggr", cases.scored_cases())
def test_against_the_mirror(ops, mirror, name, scheme, aggr):
    src, dst, n, ei = device_graph(name)
    E = src.size
    w = cases.weights(E)
    kw = dict(p=list(cases.PS), scheme=scheme, threshold=cases.THRESHOLD, seed=cases.SEED, aggr=aggr)
    want = edgedrop_mirror.run(mirror, src, dst, n, w=w, **kw)
    rows, ptr, mask, scores = ops.drop_edges(ei, torch.from_numpy(w).cuda(), n, return_mask=True, return_scores=True, **kw)
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["rows_needed"] == rows.shape[0]
    got_c, got_nw = scores["centrality"].cpu().numpy(), scores["node_weight"].cpu().numpy()
    assert np.array_equal(bits(got_c), bits(want["centrality"])), f"centrality differs at {np.flatnonzero(got_c != want['centrality'])[:5]}"
    assert (scores["iters"], scores["converged"]) == (want["iters"], want["converged"])
    if scheme != "uniform":
        cnt = np.bincount(src if aggr == "source" else dst, minlength=n)
        on = cnt > 0
        if name == "ring64":
            assert np.isnan(got_nw).all()
        else:
            s = np.log(want["centrality"][on])
            smax, smean = s.max(), float((cnt[on] * s).sum() / E)
            bound = 8 * 2.0 ** -52 * np.abs(s).max() / (smax - smean)
            diff = np.abs(got_nw[on] - want["node_weight"][on]).max()
            print(f"{name} {scheme} {aggr}: max node_weight difference {diff:.3e}, bound {bound:.3e}")
            assert diff <= bound
            off = ~on
            assert np.array_equal(np.isfinite(got_nw[off]), np.isfinite(want["node_weight"][off]))
    else:
        assert not got_c.any() and not got_nw.any()
    m = mask.cpu().numpy()
    outside = np.abs(want["u"] - want["q"]) > cases.BAND
    assert outside.all() and np.array_equal(m[outside], want["mask"][outside])
    exp_rows, exp_ptr = expected_rows(src, dst, w, m)
    assert ptr.tolist() == exp_ptr and np.array_equal(bits(rows.cpu().numpy()), bits(exp_rows))     # the weights reach column 2 untouched
    if name == "ring64" and scheme != "uniform":
        assert np.array_equal(m, want["u"] >= cases.THRESHOLD)


@pytest.mark.parametrize("E", cases.TILE_EDGE_ROWS)
def test_compaction_at_the_tile_edges(ops, mirror, E):
    src, dst, n = cases.random_rows(E)
    ei = torch.from_numpy(np.stack([src, dst])).cuda()
    for K in (1, 2, 3):
        for aggr in ("sink", "source"):
            want = edgedrop_mirror.run(mirror, src, dst, n, p=[0.5] * K, scheme="uniform", seed=cases.SEED, aggr=aggr)
            rows, ptr, mask = ops.drop_edges(ei, None, n, [0.5] * K, "uniform", seed=cases.SEED, aggr=aggr, return_mask=True)
            assert tuple(mask.shape) == (K, E) and np.array_equal(mask.cpu().numpy(), want["mask"])
            assert ptr.tolist() == want["ptr"].tolist() and np.array_equal(rows.cpu().numpy(), want["rows"])
    if E > cases.ROW_TILE:                                                          # a scored scheme across several row tiles
        want = edgedrop_mirror.run(mirror, src, dst, n, p=[0.3, 0.6], scheme="degree", seed=cases.SEED, aggr="source")
        assert (np.abs(want["u"] - want["q"]) > cases.BAND).all()
        rows, ptr = ops.drop_edges(ei, None, n, [0.3, 0.6], "degree", seed=cases.SEED, aggr="source")
        assert ptr.tolist() == want["ptr"].tolist() and np.array_equal(rows.cpu().numpy(), want["rows"])


@pytest.mark.parametrize("scheme", cases.SCHEMES)
def test_views_repeats_and_empty_views(ops, mirror, scheme):
    src, dst, n, ei = device_graph("ba300")
    E = src.size
    ps = [0.2, 0.5, 0.35]
    rows, ptr, mask = ops.drop_edges(ei, None, n, ps, scheme, seed=40, return_mask=True)
    again = ops.drop_edges(ei, None, n, ps, scheme, seed=40, return_mask=True)
    assert all(torch.equal(a, b) for a, b in zip((rows, ptr, mask), again))          # a repeated call returns equal bits
    p = ptr.tolist()
    for k in range(3):
        r1, p1, m1 = ops.drop_edges(ei, None, n, ps[k], scheme, seed=40 + k, return_mask=True)
        assert torch.equal(m1[0], mask[k]) and torch.equal(r1, rows[p[k]:p[k + 1]]) and p1.tolist() == [0, p[k + 1] - p[k]]
    rows, ptr, mask = ops.drop_edges(ei, None, n, [0.0, 0.0], scheme, seed=3, return_mask=True)
    assert mask.all() and ptr.tolist() == [0, E, 2 * E] and torch.equal(rows[:E, :2].long().t(), ei) and bool((rows[:, 2] == 1.0).all())
    if scheme == "uniform":
        rows, ptr, mask = ops.drop_edges(ei, None, n, [1.0, 0.0, 1.0], scheme, return_mask=True)
        assert ptr.tolist() == [0, 0, E, E] and not mask[0].any() and not mask[2].any() and rows.shape[0] == E   # empty views: equal offsets
    none = ops.drop_edges(torch.zeros((2, 0), dtype=torch.int64, device="cuda"), None, 5, [0.5, 0.5], scheme, pr_iters=7, return_scores=True)
    assert tuple(none[0].shape) == (0, 3) and none[1].tolist() == [0, 0, 0] and not none[2]["centrality"].any()
    empty = np.zeros(0, dtype=np.int64)
    want = edgedrop_mirror.run(mirror, empty, empty, 5, p=[0.5, 0.5], scheme=scheme, pr_iters=7)   # no rows: the same report as the mirror
    assert (none[2]["iters"], none[2]["converged"]) == (want["iters"], want["converged"]) == (7 if scheme == "pagerank" else 0, True)


def test_refusals_and_the_convergence_report(ops):
    src, dst, n, ei = device_graph("ba300")
    with pytest.raises(ValueError, match="out of range"):
        ops.drop_edges(ei, None, n - 1, 0.5, "degree")
    bad = ei.clone()
    bad[1, 7] = -1
    for scheme in cases.SCHEMES:
        with pytest.raises(ValueError):
            ops.drop_edges(bad, None, n, 0.5, scheme)
    for kw in (dict(p=[0.5] * 33), dict(p=1.5), dict(scheme="katz")):
        with pytest.raises(ValueError):
            ops.drop_edges(ei, None, n, **kw)
    rows, ptr = ops.drop_edges(ei, None, n, 0.5, "degree")                            # the handle works after the refusals
    assert 0 < rows.shape[0] < src.size and ptr.tolist() == [0, rows.shape[0]]
    scores = ops.drop_edges(ei, None, n, 0.5, "eigenvector", evc_tol=1e-12, evc_max_iter=3, return_scores=True)[2]
    assert (scores["iters"], scores["converged"]) == (3, False)
    scores = ops.drop_edges(ei, None, n, 0.5, "eigenvector", return_scores=True)[2]
    assert scores["converged"] and 3 < scores["iters"] < 1000


def test_plan_of_the_views_through_the_layer(ops):
    from rlap_amd import adapters
    src, dst, n, ei = device_graph("ba300")
    torch.manual_seed(0)
    x = torch.randn(n, 8, dtype=torch.float64, device="cuda")
    views = adapters.EdgeDroppingViews("degree", (0.3, 0.45), 0.7)
    plan = views.plan(adapters.Graph(x, ei, None))
    _, _, mask = ops.drop_edges(ei, None, n, [0.3, 0.45], "degree", 0.7, seed=views.last_seed, return_mask=True)   # the call's own seed
    kept = [ei[:, mask[k]] for k in range(2)]
    rows = torch.cat([torch.stack([e[0].double(), e[1].double(), torch.ones(e.shape[1], dtype=torch.float64, device="cuda")], 1) for e in kept])
    ref = ops.edge_list_plan(rows, [0, kept[0].shape[1], kept[0].shape[1] + kept[1].shape[1]], n)
    assert plan.layers == 2 and 0 < kept[0].shape[1] < src.size
    conv = adapters.SnapshotGCNConv(8, 4).double().cuda()
    out = conv(x, plan)
    assert tuple(out.shape) == (2, n, 4) and torch.equal(out, conv(x, ref))
    out.sum().backward()
    assert conv.weight.grad is not None and bool(conv.weight.grad.abs().sum() > 0)
    fixed = adapters.EdgeDroppingViews("degree", (0.3, 0.45), 0.7, views.last_seed)   # an explicit seed repeats the views
    g1, g2 = (aug(x, ei, None) for aug in fixed.augmentors())
    assert torch.equal(g1.edge_index, kept[0]) and torch.equal(g2.edge_index, kept[1]) and g1.edge_weights is None
    one = adapters.EdgeDroppingDegree(0.3, 0.7, views.last_seed)(x, ei, None)         # max id + 1 nodes, as the reference: the same graph here
    assert torch.equal(one.edge_index, kept[0])


def test_default_augmentors_give_independent_views(ops):
    """The reference's (aug1, aug2) are built with the same arguments and called at every step: without an explicit seed neither the
    two augmentors nor two calls of one return the same view, and the kept share is what p asks for."""
    from rlap_amd import adapters
    src, dst, n, ei = device_graph("ba300")
    E = src.size
    for cls in (adapters.EdgeDropping, adapters.EdgeDroppingDegree, adapters.EdgeDroppingPR, adapters.EdgeDroppingEVC):
        aug1, aug2 = (cls(0.3), cls(0.3)) if cls is adapters.EdgeDropping else (cls(0.3, 0.7), cls(0.3, 0.7))
        views = [aug1(None, ei).edge_index, aug2(None, ei).edge_index, aug1(None, ei).edge_index]
        assert all(0.5 * E < v.shape[1] < 0.95 * E for v in views)                  # q <= threshold = 0.7 and its mean is at most p = 0.3
        assert not any(a.shape == b.shape and torch.equal(a, b) for i, a in enumerate(views) for b in views[i + 1:])
    pair = adapters.EdgeDroppingViews("pagerank", (0.3, 0.3), 0.7)
    g1, g2 = (aug(None, ei) for aug in pair.augmentors())
    h1, _ = (aug(None, ei) for aug in pair.augmentors())
    assert not (g1.edge_index.shape == g2.edge_index.shape and torch.equal(g1.edge_index, g2.edge_index))
    assert not (g1.edge_index.shape == h1.edge_index.shape and torch.equal(g1.edge_index, h1.edge_index))
