"""Edge dropping on the device where tests/test_gpu_edge_drop.py does not reach, against the same host mirror and by
the same comparisons: centrality, mask, rows and ptr by equality of bits, node_weight within 8 * 2^-52 * max|s| / (smax - smean),
one host synchronisation a call.  tests/test_edge_drop_cpu.py asserts on these very inputs that no coin lies within BAND of its
drop probability, so the mask comparison leaves out no row.

  * node tiles and key widths: N = 255, 256, 257, 65,536 and 65,537 -- 1, 1, 2, 256 and 257 tiles of 256 nodes, so wg_total's lanes
    make one full trip at 65,536 and lane 0 a second one at 65,537, whose sum must equal the header's total_reduce bit for bit; N on
    both sides of a power of two with the top id at both ends of rows, where key_bits and pair_key_bits decide whether the radix
    sort sees the top bit;
  * sorted row lists: run_add, the wave-run counter behind in[], out[] and the degree count, on rows sorted by target and by source:
    runs that start on lane 0, end on lane 63, fill a wave, cross the workgroup's edge, and the same runs moved on by one lane;
  * K = 32: every view the flip kernels keep a wave count for.

Measured on an MI355X: the largest node_weight difference of the node-tile cases is 8.9e-16 (N = 257, pagerank by target, bound
5.8e-15; N = 65,536, eigenvector, bounds 1.2e-14 and 9.8e-15), 0 in 14 of the 30 scored ones and in all 16 of the sorted row
lists."""
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
    return edgedrop_mirror.build(tmp_path_factory.mktemp("edgedrop_regimes"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def expected_rows(src, dst, w, mask):
    parts = [np.stack([src[m], dst[m], (w[m] if w is not None else np.ones(int(m.sum())))], 1) for m in mask]
    return np.concatenate(parts).reshape(-1, 3), [0] + np.cumsum(mask.sum(1)).tolist()


def against_the_mirror(ops, mirror, what, src, dst, n, w, scheme, aggr, **kw):
    """One call on the device and by the mirror, compared as tests/test_gpu_edge_drop.py::test_against_the_mirror compares them.
    Returns the mirror's dict."""
    E = src.size
    kw = dict(p=list(cases.PS), scheme=scheme, threshold=cases.THRESHOLD, seed=cases.SEED, aggr=aggr, **kw)
    want = edgedrop_mirror.run(mirror, src, dst, n, w=w, **kw)
    ei = torch.from_numpy(np.stack([src, dst])).cuda()
    rows, ptr, mask, scores = ops.drop_edges(ei, torch.from_numpy(w).cuda(), n, return_mask=True, return_scores=True, **kw)
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["rows_needed"] == rows.shape[0]
    got_c, got_nw = scores["centrality"].cpu().numpy(), scores["node_weight"].cpu().numpy()
    assert np.array_equal(bits(got_c), bits(want["centrality"])), f"{what}: centrality differs at {np.flatnonzero(got_c != want['centrality'])[:5]}"
    assert (scores["iters"], scores["converged"]) == (want["iters"], want["converged"])
    if scheme != "uniform":
        cnt = np.bincount(src if aggr == "source" else dst, minlength=n)
        on = cnt > 0
        s = np.log(want["centrality"][on])
        smax, smean = s.max(), float((cnt[on] * s).sum() / E)
        assert smax > smean                                                         # (no case here is degenerate as the ring is)
        bound = 8 * 2.0 ** -52 * np.abs(s).max() / (smax - smean)
        diff = np.abs(got_nw[on] - want["node_weight"][on]).max()
        print(f"{what} {scheme} {aggr}: max node_weight difference {diff:.3e}, bound {bound:.3e}")
        assert diff <= bound
        off = ~on
        assert np.array_equal(np.isfinite(got_nw[off]), np.isfinite(want["node_weight"][off]))
    else:
        assert not got_c.any() and not got_nw.any()
    m = mask.cpu().numpy()
    gap = np.abs(want["u"] - want["q"])
    assert gap.min() > cases.BAND, f"{what}: a coin inside the band ({gap.min():.2e})"   # every row is compared
    assert np.array_equal(m, want["mask"])
    exp_rows, exp_ptr = expected_rows(src, dst, w, m)
    assert ptr.tolist() == exp_ptr == want["ptr"].tolist() and np.array_equal(bits(rows.cpu().numpy()), bits(exp_rows))
    return want


@pytest.mark.parametrize("scheme", cases.SCHEMES)
@pytest.mark.parametrize("n", cases.NODE_EDGE_NODES)
def test_node_tiles_and_key_widths(ops, mirror, n, scheme):
    src, dst, _ = cases.node_edge_rows(n)
    w = cases.weights(src.size)
    for aggr in ("sink", "source"):
        want = against_the_mirror(ops, mirror, f"n = {n}", src, dst, n, w, scheme, aggr, **cases.NODE_EDGE_ITERS)
        if scheme == "eigenvector":
            assert (want["iters"], want["converged"]) == (5, False)
        if scheme != "uniform":
            assert want["centrality"][n - 1] > 0                                    # the top id has rows at both ends: it is scored


@pytest.mark.parametrize("scheme", ("pagerank", "degree"))
@pytest.mark.parametrize("variant", list(cases.RUN_VARIANTS))
def test_sorted_row_lists(ops, mirror, variant, scheme):
    src, dst, n = cases.runs(*cases.RUN_VARIANTS[variant])
    w = cases.weights(src.size)
    for aggr in ("sink", "source"):
        against_the_mirror(ops, mirror, f"runs {variant}", src, dst, n, w, scheme, aggr)


@pytest.mark.parametrize("scheme", ("uniform", "degree"))
def test_thirty_two_views(ops, mirror, scheme):
    src, dst, n = cases.random_rows(cases.ROW_TILE + 1)
    ei = torch.from_numpy(np.stack([src, dst])).cuda()
    ps = list(cases.MANY_PS)
    kw = dict(scheme=scheme, threshold=cases.THRESHOLD)
    want = edgedrop_mirror.run(mirror, src, dst, n, p=ps, seed=cases.SEED, **kw)
    assert (np.abs(want["u"] - want["q"]) > cases.BAND).all()
    rows, ptr, mask = ops.drop_edges(ei, None, n, ps, seed=cases.SEED, return_mask=True, **kw)
    assert ops.last_stats["host_syncs"] == 1 and tuple(mask.shape) == (32, src.size)
    assert np.array_equal(mask.cpu().numpy(), want["mask"])
    assert ptr.tolist() == want["ptr"].tolist() and np.array_equal(bits(rows.cpu().numpy()), bits(want["rows"]))
    p = ptr.tolist()
    for k in (0, 31):
        r1, p1, m1 = ops.drop_edges(ei, None, n, ps[k], seed=cases.SEED + k, return_mask=True, **kw)
        assert torch.equal(m1[0], mask[k]) and torch.equal(r1, rows[p[k]:p[k + 1]]) and p1.tolist() == [0, p[k + 1] - p[k]]
