"""PPR diffusion of snapshots on the device (ops.snapshot_ppr, ops.ppr_diffusion, rlap_ppr.hip) across both step
parities, both regimes and the group limits, each against a dense float64 inverse (tests/ppr_dense.py):

  a. even and odd step counts K at four alphas, K = 0, 1 and 2 against their closed forms, an even K in the large regime;
  b. segments of 1, 2, 63, 64, 65, 128 and 129 nodes, a hub block of 199 rows and hubs of 4 to 7 rows, in one call and alone;
  c. 4,096 nodes (the last size of the one-workgroup regime) and 4,097 (the first of the one-launch-per-step regime);
  d. groups closed by the tile budget in either regime and by the tile count, the output offset carried from group to group;
  e. the output retry of the Python layer;
  f. ids without edges and without a self loop;
  g. every call is made twice and gives the same bits.

The yardstick: before normalisation every kept entry lies within 2 tol of the exact one (rlap_cheb.h proves ||x - x_K||_2 <=
1 / T_K(mu) <= tol; the factor 2 leaves room for float64 rounding, of the order K d_max 2^-53, far below every tol >= 1e-12 used
here), and the keep pattern is exactly S0 >= eps -- every test first asserts that no exact entry lies within 2 tol of eps, so the
reference alone decides it.  Normalised output: rtol = 1e-7, atol = 1e-12 at tol = 1e-12, as tests/test_gpu_ppr.py.

At alpha = 0.2 that yardstick cannot tell x_K from x_{K-1} (T_K / T_{K-1} is about 2, the observed error a few per cent of tol), so
raw output is also compared with the dense recurrence of rlap_cheb.h itself (check_iterate): it must lie four times closer to x_K
than x_{K-1} does.

Every test prints its largest err / tol.  Observed on an MI355X (largest err / tol per test):
  a. BA(300, 4), without / with the self loop: (0.2, 1e-11) 0.036 / 0.035; (0.2, 1e-8) 0.041 / 0.057; (0.2, 1e-10) 0.027 / 0.030;
     (0.05, 1e-10) 0.018 / 0.015; (0.05, 1e-9) 0.018 / 0.017; (0.5, 1e-11) 0.12 / 0.11; (0.85, 1e-12) 0.23 / 0.29;
     (0.85, 1e-10) 0.046 / 0.040; 4,100 nodes at K = 38: 0.10
  b. K = 35 / 38: one loop row 0.58 / 0.73 (its one eigenvalue is 1 - alpha, where the bound is attained); two nodes 0.32 / 0.40;
     the stars 0.26 / 0.40; 63 to 129 nodes 0.036 to 0.097 / 0.043 to 0.12
  c. 4,096 nodes 0.025, 4,097 nodes 0.028 (K = 41)
  d. two nodes 0.32      e. the star of 2,100 nodes 0.26 at both eps
  against the recurrence: |out - x_K| <= 5.6e-16 everywhere; the smallest |x_K - x_{K-1}| among the kept entries is 2.3e-13 (4,097
  nodes, K = 41), 6.4e-13 on BA(300, 4) (alpha = 0.2, K = 38)
"""
import numpy as np
import pytest
import torch

from ppr_dense import chebyshev_iterates, dense_ppr, system, threshold, to_dense
from test_gpu_ppr import sc_of
from util import ba_graph, path, star

pytestmark = pytest.mark.gpu

EPS = 1e-4


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def ppr_twice(ops, sc, ptr, n, **kw):
    """(out, pptr, last_stats) of ops.snapshot_ppr; the call is made twice and must give the same bits (g)."""
    out, pptr = ops.snapshot_ppr(sc, ptr, n, **kw)
    st = dict(ops.last_stats)
    out2, pptr2 = ops.snapshot_ppr(sc, ptr, n, **kw)
    assert same_bits(out, out2) and torch.equal(pptr, pptr2), "the same call gave other bits"
    return out, pptr, st


def exact(sc, alpha=0.2, self_loop=False):
    """(sorted ids, S before the threshold) of one segment."""
    nodes, S0, _ = dense_ppr(sc, alpha=alpha, eps=1.0, self_loop=self_loop, normalize=False)
    return nodes, S0


def row_major(out, nodes):
    key = out[:, 0].long() * (int(nodes.max()) + 1) + out[:, 1].long()
    assert bool((key[1:] > key[:-1]).all()), "rows are not in ascending (i, j) order"


def determined(S0, tol, eps):
    assert not np.any(np.abs(S0 - eps) <= 2 * tol), "an exact entry lies within 2 tol of eps: the keep decision is not determined"


def check_raw(what, out, nodes, S0, tol, eps=EPS):
    """Output before normalisation against the exact matrix: the keep pattern exactly, every kept entry within 2 tol."""
    determined(S0, tol, eps)
    got, keep = to_dense(out, nodes)
    assert np.array_equal(keep, S0 >= eps), "the keep pattern differs from S0 >= eps"
    err = float(np.abs(got - S0)[keep].max()) if keep.any() else 0.0
    print(f"{what}: max err / tol = {err / tol:.3g}")
    assert err <= 2 * tol
    row_major(out, nodes)


def check_iterate(what, out, sc, alpha, K, self_loop=False, on_device=False):
    """The 2 tol yardstick cannot tell x_K from x_{K-1} (at alpha = 0.2, T_K / T_{K-1} is about 2 and the observed error a few per
    cent of tol), so the output before normalisation is also compared with the dense recurrence itself: it differs from x_K by
    rounding alone (of the order K 2^-53 per entry, 1e-14 here) and must lie at least four times closer to it than x_{K-1} does
    where they differ most among the kept entries -- a wrong parity returns x_{K-1}, or zeros, and fails."""
    nodes, Ahat = system(sc, self_loop=self_loop)
    xp, x = chebyshev_iterates(torch.from_numpy(Ahat).cuda() if on_device else Ahat, alpha, K)   # (4,100 nodes take too long in numpy)
    got, keep = to_dense(out, nodes)
    gap = float(np.abs(x - xp)[keep].max())
    d = float(np.abs(got - x)[keep].max())
    print(f"{what}: |out - x_K| = {d:.3g}, |x_K - x_(K-1)| = {gap:.3g}")
    assert gap > 0.0 and d <= gap / 4


def check_normalised(out, nodes, S0, eps=EPS):
    """Normalised output of a call with tol = 1e-12 against the dense adapter's formula."""
    determined(S0, 1e-12, eps)
    got, keep = to_dense(out, nodes)
    assert np.array_equal(keep, S0 >= eps)
    assert np.allclose(got, threshold(S0, eps), rtol=1e-7, atol=1e-12)
    row_major(out, nodes)


# ------------------------------------------------------------------------------------------------ a. step parity and alpha
PAIRS = [(0.2, 1e-11, 38), (0.2, 1e-8, 28), (0.2, 1e-10, 35), (0.05, 1e-10, 74), (0.05, 1e-9, 67), (0.5, 1e-11, 20), (0.85, 1e-12, 11),
         (0.85, 1e-10, 10)]


@pytest.fixture(scope="module")
def ba300():
    return sc_of(ba_graph(300, 4, 21))


def test_the_pairs_hold_both_parities(ops):
    assert {K & 1 for _, _, K in PAIRS} == {0, 1}
    assert {K & 1 for a, _, K in PAIRS if a == 0.2} == {0, 1}
    for alpha, tol, K in PAIRS:
        assert ops.ppr_steps(alpha, tol) == K
    assert [ops.ppr_steps(0.2, t) for t in (1.0, 0.9, 0.5)] == [0, 1, 2]


@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("alpha,tol,K", PAIRS)
def test_step_parity_and_alpha(ops, ba300, alpha, tol, K, self_loop):
    sc = ba300
    out, pptr, st = ppr_twice(ops, sc, [0, sc.shape[0]], 300, alpha=alpha, tol=tol, add_self_loop=self_loop, normalize_out=False)
    assert st["steps"] == K == ops.ppr_steps(alpha, tol)
    assert (st["small_tiles"], st["large_tiles"], st["groups"]) == (5, 0, 1)
    assert pptr.tolist() == [0, out.shape[0]]
    nodes, S0 = exact(sc, alpha, self_loop)
    check_raw(f"alpha={alpha} tol={tol} K={K} self_loop={self_loop}", out, nodes, S0, tol)
    check_iterate(f"alpha={alpha} K={K} self_loop={self_loop}", out, sc, alpha, K, self_loop)


@pytest.mark.parametrize("normalize", [False, True])
def test_no_step_keeps_nothing(ops, ba300, normalize):
    """tol >= 1: K = 0, x_0 = 0 -- no entry reaches eps."""
    sc = ba300
    out, pptr, st = ppr_twice(ops, torch.cat([sc, sc]), [0, sc.shape[0], 2 * sc.shape[0]], 300, tol=1.0, normalize_out=normalize)
    assert st["steps"] == 0 and st["rows_needed"] == 0
    assert out.shape == (0, 3) and pptr.tolist() == [0, 0, 0]


@pytest.mark.parametrize("self_loop", [False, True])
def test_one_step_is_the_diagonal(ops, ba300, self_loop):
    """K = 1: x_1 = f = alpha e_j, whatever the graph."""
    sc = ba300
    out, pptr, st = ppr_twice(ops, sc, [0, sc.shape[0]], 300, alpha=0.2, tol=0.9, add_self_loop=self_loop, normalize_out=False)
    assert st["steps"] == 1
    ids = torch.arange(300, dtype=torch.float64, device=out.device)
    want = torch.stack([ids, ids, torch.full_like(ids, 0.2)], 1)
    assert same_bits(out, want) and pptr.tolist() == [0, 300]
    out, _, _ = ppr_twice(ops, sc, [0, sc.shape[0]], 300, alpha=0.2, tol=0.9, add_self_loop=self_loop)
    assert torch.equal(out[:, :2], want[:, :2])
    assert float((out[:, 2] - 1.0).abs().max()) <= 2.0 ** -51                  # 0.2 (0.2^-1/2)^2 in three roundings
    out, pptr, _ = ppr_twice(ops, sc, [0, sc.shape[0]], 300, alpha=0.2, eps=0.25, tol=0.9, add_self_loop=self_loop)
    assert out.shape == (0, 3) and pptr.tolist() == [0, 0]                     # alpha < eps


@pytest.mark.parametrize("self_loop", [False, True])
def test_two_steps_closed_form(ops, ba300, self_loop):
    """K = 2: x_2 = om_1 (B f + f) with om_1 = 2 mu^2 / (2 mu^2 - 1), mu = 1 / (1 - alpha), B = (1 - alpha) D^-1/2 A D^-1/2."""
    sc = ba300
    alpha = 0.2
    out, pptr, st = ppr_twice(ops, sc, [0, sc.shape[0]], 300, alpha=alpha, tol=0.5, add_self_loop=self_loop, normalize_out=False)
    assert st["steps"] == 2
    part = sc.cpu().numpy()
    A = np.zeros((300, 300))
    A[part[:, 0].astype(int), part[:, 1].astype(int)] = part[:, 2]
    if self_loop:
        A += np.eye(300)
    dinv = A.sum(1) ** -0.5
    mu = 1.0 / (1.0 - alpha)
    om1 = 2.0 * mu * mu / (2.0 * mu * mu - 1.0)
    X2 = om1 * ((1.0 - alpha) * (dinv[:, None] * A * dinv[None, :]) * alpha + alpha * np.eye(300))
    assert not np.any(np.abs(X2 - EPS) <= 1e-12)
    got, keep = to_dense(out, np.arange(300))
    assert np.array_equal(keep, X2 >= EPS) and keep.sum() == out.shape[0] == pptr.tolist()[1]
    # a kept entry is a product of at most eight correctly rounded operations on either side: 16 * 2^-53 < 1e-14 relative
    assert np.allclose(got, np.where(keep, X2, 0.0), rtol=1e-14, atol=0.0)
    row_major(out, np.arange(300))


class Segment:
    """A plain graph as one segment: its rows on the device, its exact matrix (computed once), and its result alone."""

    def __init__(self, ei, alpha=0.2):
        self.sc = sc_of(ei)
        self.m = self.sc.shape[0]
        self.n = int(ei.max()) + 1
        self.nodes, self.S0 = exact(self.sc, alpha)
        assert len(self.nodes) == self.n
        self.alone = {}

    def run(self, ops, **kw):
        """(out, last_stats) of the segment alone, once per set of arguments."""
        key = tuple(sorted(kw.items()))
        if key not in self.alone:
            out, pptr, st = ppr_twice(ops, self.sc, [0, self.m], self.n, **kw)
            assert pptr.tolist() == [0, out.shape[0]]
            self.alone[key] = (out, st)
        return self.alone[key]

    def times(self, k):
        """The segment k times as k segments of one call: (sc, ptr)."""
        return torch.cat([self.sc] * k), [self.m * s for s in range(k + 1)]


def same_as_alone(out, pptr, alone):
    pp = pptr.tolist()
    assert pp[0] == 0 and pp[-1] == out.shape[0]
    for s in range(len(pp) - 1):
        assert same_bits(out[pp[s]:pp[s + 1]], alone), f"segment {s} differs from the segment alone"


@pytest.fixture(scope="module")
def seg4100():
    return Segment(ba_graph(4100, 3, 3))


EVEN = dict(tol=1e-11, normalize_out=False)   # K = 38


def test_even_step_count_in_the_large_regime(ops, seg4100):
    g = seg4100
    out, st = g.run(ops, **EVEN)
    assert st["steps"] == 38 and (st["small_tiles"], st["large_tiles"], st["groups"]) == (0, 65, 1)
    check_raw("4100 nodes, K=38", out, g.nodes, g.S0, 1e-11)
    check_iterate("4100 nodes, K=38", out, g.sc, 0.2, 38, on_device=True)


# ------------------------------------------------------------------------------------------------ b. tile edges
def edge_graphs():
    loop = np.array([[0], [0]], dtype=np.int64)                                # one node, one loop row
    return [loop, path(2), path(63), ba_graph(64, 3, 1), ba_graph(65, 3, 2), path(128), ba_graph(129, 3, 3), star(200), star(5), star(6),
            star(7), star(8), path(64), ba_graph(128, 4, 4)]


EDGE_NODES = [1, 2, 63, 64, 65, 128, 129, 200, 5, 6, 7, 8, 64, 128]


@pytest.mark.parametrize("tol,K", [(1e-10, 35), (1e-11, 38)])
def test_tile_edges_alone_and_together(ops, tol, K):
    parts = [sc_of(g) for g in edge_graphs()]
    assert [len(torch.unique(p[:, :2])) for p in parts] == EDGE_NODES
    hub_rows = [int((p[:, 1] == 0).sum()) for p in parts]
    assert hub_rows[7:12] == [199, 4, 5, 6, 7]                                  # 49 * 4 + 3 and every remainder of the 4-way gather
    sc = torch.cat(parts)
    ptr = np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).tolist()
    out, pptr, st = ppr_twice(ops, sc, ptr, 200, tol=tol, normalize_out=False)
    assert st["steps"] == K and st["small_tiles"] == sum(-(-n // 64) for n in EDGE_NODES) and st["large_tiles"] == 0 and st["groups"] == 1
    pp = pptr.tolist()
    assert pp[-1] == out.shape[0]
    for s, p in enumerate(parts):
        alone, ap, st1 = ppr_twice(ops, p, [0, p.shape[0]], 200, tol=tol, normalize_out=False)
        assert st1["small_tiles"] == -(-EDGE_NODES[s] // 64)
        assert same_bits(out[pp[s]:pp[s + 1]], alone) and ap.tolist() == [0, pp[s + 1] - pp[s]], s
        nodes, S0 = exact(p)
        check_raw(f"{EDGE_NODES[s]} nodes (segment {s}), K={K}", alone, nodes, S0, tol)
        check_iterate(f"{EDGE_NODES[s]} nodes (segment {s}), K={K}", alone, p, 0.2, K)
    # normalised, at the tolerance the bound of test_gpu_ppr.py is stated for
    out, pptr, _ = ppr_twice(ops, sc, ptr, 200, tol=1e-12)
    pp = pptr.tolist()
    for s, p in enumerate(parts):
        nodes, S0 = exact(p)
        check_normalised(out[pp[s]:pp[s + 1]], nodes, S0)


# ------------------------------------------------------------------------------------------------ c. the regime edge
@pytest.fixture(scope="module")
def edge_segments():
    return {4096: Segment(ba_graph(4096, 3, 6)), 4097: Segment(ba_graph(4097, 3, 1))}


RAW12 = dict(tol=1e-12, normalize_out=False)


@pytest.mark.parametrize("n,small,large", [(4096, 64, 0), (4097, 0, 65)])
def test_regime_edge_against_the_inverse(ops, edge_segments, n, small, large):
    g = edge_segments[n]
    out, st = g.run(ops, **RAW12)
    assert st["steps"] == 41 and (st["small_tiles"], st["large_tiles"], st["groups"]) == (small, large, 1)
    check_raw(f"{n} nodes, K=41", out, g.nodes, g.S0, 1e-12)
    check_iterate(f"{n} nodes, K=41", out, g.sc, 0.2, 41, on_device=True)
    out, st = g.run(ops, tol=1e-12)
    assert (st["small_tiles"], st["large_tiles"], st["groups"]) == (small, large, 1)
    check_normalised(out, g.nodes, g.S0)
    i, j, v = out[:, 0].long(), out[:, 1].long(), out[:, 2]
    kf, of = torch.sort(i * n + j)
    kb, ob = torch.sort(j * n + i)
    assert torch.equal(kf, kb) and same_bits(v[of], v[ob])                      # exactly symmetric
    assert bool((v > 0).all())
    assert torch.equal(i[i == j], torch.arange(n, device=i.device))             # the diagonal holds every node


# ------------------------------------------------------------------------------------------------ d. groups
def test_groups_by_the_budget_large_regime(ops, seg4100):
    """4 x 65 tiles of 4.2 MB exceed 1 GiB: the fourth segment's last tiles open a second group."""
    g = seg4100
    alone, _ = g.run(ops, **EVEN)
    sc, ptr = g.times(4)
    out, pptr, st = ppr_twice(ops, sc, ptr, g.n, **EVEN)
    assert (st["groups"], st["large_tiles"], st["small_tiles"]) == (2, 260, 0)
    assert pptr.tolist() == [alone.shape[0] * s for s in range(5)]
    same_as_alone(out, pptr, alone)


def test_groups_by_the_budget_small_regime(ops, edge_segments):
    """5 x 64 tiles of 4 MiB: exactly 256 fill the budget, the fifth segment is a second group."""
    g = edge_segments[4096]
    alone, _ = g.run(ops, **RAW12)
    sc, ptr = g.times(5)
    out, pptr, st = ppr_twice(ops, sc, ptr, g.n, **RAW12)
    assert (st["groups"], st["small_tiles"], st["large_tiles"]) == (2, 320, 0)
    assert pptr.tolist() == [alone.shape[0] * s for s in range(6)]
    same_as_alone(out, pptr, alone)


def test_groups_by_the_tile_count(ops):
    """66,000 one-tile segments: a group ends at 65,535 tiles."""
    S = 66_000
    two = sc_of(np.array([[0, 1], [1, 0]]), [2.0, 2.0])
    alone, ap, st1 = ppr_twice(ops, two, [0, 2], 2)
    assert ap.tolist() == [0, 4] and (st1["groups"], st1["small_tiles"]) == (1, 1)
    nodes, S0 = exact(two)
    determined(S0, 1e-10, EPS)
    raw, _, _ = ppr_twice(ops, two, [0, 2], 2, normalize_out=False)
    check_raw("two nodes", raw, nodes, S0, 1e-10)
    out, pptr, st = ppr_twice(ops, two.repeat(S, 1), list(range(0, 2 * S + 1, 2)), 2)
    assert (st["groups"], st["small_tiles"], st["large_tiles"], st["rows_needed"]) == (2, S, 0, 4 * S)
    assert torch.equal(pptr.cpu(), 4 * torch.arange(S + 1))
    assert same_bits(out.reshape(S, 4, 3), alone.unsqueeze(0).expand(S, 4, 3))


# ------------------------------------------------------------------------------------------------ e. the output retry
def test_output_retry(ops):
    """A star of 2,100 nodes at eps = 1e-5 keeps all 4,410,000 pairs: more than the first capacity, max(16 m + 64, 2^22)."""
    n = 2100
    g = Segment(star(n))
    assert float(g.S0.min()) > 1.6e-4 and n * n > max(16 * g.m + 64, 1 << 22)
    out, st = g.run(ops, eps=1e-5, normalize_out=False)
    assert st["output_retries"] == 1 and st["rows_needed"] == 4_410_000 == out.shape[0]
    assert st["first_cap"] == 1 << 22
    check_raw("star of 2100, eps=1e-5", out, g.nodes, g.S0, 1e-10, eps=1e-5)
    out, st = g.run(ops, eps=1e-3, normalize_out=False)
    assert st["output_retries"] == 0 and st["rows_needed"] == out.shape[0] == int((g.S0 >= 1e-3).sum())
    check_raw("star of 2100, eps=1e-3", out, g.nodes, g.S0, 1e-10, eps=1e-3)


# ------------------------------------------------------------------------------------------------ f. zero rows
def diffusion_twice(ops, *a, **kw):
    ei, w = ops.ppr_diffusion(*a, **kw)
    ei2, w2 = ops.ppr_diffusion(*a, **kw)
    assert torch.equal(ei, ei2) and same_bits(w, w2)
    return ei, w


@pytest.mark.parametrize("alpha,tol,K,exact_one", [(0.25, 5e-13, 37, True), (0.2, 1e-12, 41, False)])
def test_ids_without_edges_and_no_self_loop(ops, alpha, tol, K, exact_one):
    """(i, i, 0) alone is the column of an id without edges: degree 0, dinv = 0, so x_k = om (alpha - x_{k-2}) + x_{k-2} is alpha for
    every odd k, exactly (both cases have an odd K), and nothing else is in its row.  After normalisation the entry is
    alpha (alpha^-1/2)^2 in float64: exactly 1 where alpha is a power of 4 (0.25), one rounding step above 1 at alpha = 0.2 -- in
    adapters.compute_ppr as well."""
    from rlap_amd.adapters import compute_ppr
    assert ops.ppr_steps(alpha, tol) == K and K & 1
    n0 = 200
    ei = ba_graph(n0, 3, 4) + 1                    # ids 1 .. 200; 0 and 201 have no edges
    n = n0 + 2
    t = torch.from_numpy(np.ascontiguousarray(ei)).cuda()
    for normalize in (False, True):
        gi, gw = diffusion_twice(ops, t, None, n, alpha=alpha, tol=tol, normalize_out=normalize)
        assert ops.last_stats["steps"] == K
        ri, rw = compute_ppr(t, None, n, alpha=alpha, normalize_out=normalize)
        assert torch.equal(gi, ri)
        assert torch.allclose(gw, rw, rtol=1e-7, atol=1e-12)
        for v in (0, n - 1):
            row = gi[0] == v
            assert gi[1][row].tolist() == [v] and int((gi[1] == v).sum()) == 1          # the diagonal and nothing else
            d = float(gw[row][0])
            if not normalize:
                assert d == alpha
            elif exact_one:
                assert d == 1.0
            else:
                assert abs(d - 1.0) <= 2.0 ** -52
