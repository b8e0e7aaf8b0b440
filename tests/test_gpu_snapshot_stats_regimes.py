"""Snapshot statistics (ops.snapshot_stats) in both Lanczos regimes and at their limits, against graphs whose largest eigenvalue is
known in closed form (tests/spectra.py): the regime boundary at STATS_SMALL_MAX nodes, the largest LDS request of the one-workgroup
kernel, large segments stepping past the first chunk of ST_CHUNK steps and together with segments that stop at other steps, the
weighted SpMV, breakdowns, max_iter and tol on the device, and the rlap_snapshot_info report (ops.last_stats).

A converged lambda_max must match its closed form to 1e-12 relative.  Segments of one call must not see each other: every
segment's (lambda_max, iters, converged) is bit-equal to the same segment alone in its own call."""
import math

import numpy as np
import pytest
import torch

import spectra
from util import ba_graph, sym_weights, wide_weights

pytestmark = pytest.mark.gpu

SMALL_MAX = 7168   # STATS_SMALL_MAX (rlap_amd/csrc/rlap_stats.h): segments of up to this many nodes run in one workgroup
CHUNK = 32         # ST_CHUNK (rlap_stats.hip): large-regime steps enqueued between two host reads
REL = 1e-12


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def stats(ops, graphs, num_nodes=None, node_ptr=None, **kw):
    """ops.snapshot_stats over the segments `graphs` (None: empty): (per-segment results on the CPU, last_stats)."""
    sc, ptr = spectra.pack(graphs, node_ptr)
    if num_nodes is None:
        num_nodes = int(node_ptr[-1]) if node_ptr is not None else max([g.n for g in graphs if g is not None] + [1])
    st = ops.snapshot_stats(torch.from_numpy(sc).cuda(), torch.from_numpy(ptr), num_nodes, node_ptr=node_ptr, **kw)
    return {k: v.cpu() for k, v in st.items()}, dict(ops.last_stats)


def one(ops, g, **kw):
    """A single segment: (lambda_max, iters, converged, last_stats)."""
    st, info = stats(ops, [g], **kw)
    assert int(st["nodes"][0]) == g.n
    return float(st["lambda_max"][0]), int(st["iters"][0]), bool(st["converged"][0]), info


def assert_exact(lam, exact, what, rel=REL):
    assert abs(lam - exact) <= rel * exact, (what, lam, exact, abs(lam - exact) / exact)


def assert_large_report(info, iters, max_iter=1000, small=0, large=1):
    """The report of a call whose large segments took at most `iters` steps (the most of any segment)."""
    steps = min(CHUNK * math.ceil(iters / CHUNK), max_iter)
    assert info["small_segments"] == small and info["large_segments"] == large, info
    assert info["lanczos_steps"] == iters, info
    assert info["large_steps"] == steps, info
    assert info["large_launches"] == 4 * steps, info
    assert info["host_syncs"] == 3 + math.ceil(steps / CHUNK), info


# ---------------------------------------------------------------------------------------------------- a. the regime boundary

BOUNDARY = {
    # name: (builder, small regime)
    "star_7167": (lambda: spectra.star(7166), True),
    "star_7168": (lambda: spectra.star(7167), True),
    "star_7169": (lambda: spectra.star(7168), False),
    "star_7170": (lambda: spectra.star(7169), False),
    "bipartite_7167": (lambda: spectra.complete_bipartite(2, 7165), True),
    "bipartite_7168": (lambda: spectra.complete_bipartite(3, 7165), True),
    "bipartite_7169": (lambda: spectra.complete_bipartite(2, 7167), False),
    "bipartite_7170": (lambda: spectra.complete_bipartite(5, 7165), False),
    "cycle_7168": (lambda: spectra.cycle(7168), True),
    "cycle_7169": (lambda: spectra.cycle(7169), False),
    "wheel_7169": (lambda: spectra.wheel(7169), False),
    # large segments whose last tile is full (a multiple of 256 nodes) or holds one column (256 k + 1)
    "star_29x256": (lambda: spectra.star(29 * 256 - 1), False),
    "hypercube_32x256": (lambda: spectra.hypercube(13), False),
    "torus_32x256": (lambda: spectra.torus(64, 128), False),
    "star_29x256+1": (lambda: spectra.star(29 * 256), False),
    "cycle_30x256+1": (lambda: spectra.cycle(30 * 256 + 1), False),
    "tree_32x256-1": (lambda: spectra.kary_tree(2, 12), False),
}


@pytest.mark.parametrize("name", sorted(BOUNDARY))
def test_regime_boundary_alone(ops, name):
    build, small = BOUNDARY[name]
    g = build()
    lam, iters, conv, info = one(ops, g)
    assert (info["small_segments"], info["large_segments"]) == ((1, 0) if small else (0, 1)), (g.n, info)
    assert conv and info["not_converged"] == 0
    assert_exact(lam, g.lam, name)
    assert 1 <= iters <= 16, iters   # (breakdowns at step 1 or 2, or the check after them)
    if not small:
        assert_large_report(info, iters)


def test_regime_boundary_together(ops):
    names = sorted(BOUNDARY)
    gs = [BOUNDARY[k][0]() for k in names]
    st, info = stats(ops, gs)
    nsmall = sum(BOUNDARY[k][1] for k in names)
    assert info["small_segments"] == nsmall and info["large_segments"] == len(names) - nsmall, info
    assert bool(st["converged"].all())
    for s, (k, g) in enumerate(zip(names, gs)):
        assert int(st["nodes"][s]) == g.n, k
        assert_exact(float(st["lambda_max"][s]), g.lam, k)


# ---------------------------------------------------------------------------------------------------- b. the largest LDS request

def test_largest_lds_request(ops):
    # 7,168 nodes with max_iter = 1024: 16 * 7168 + 32 * 1024 bytes of dynamic LDS, the most the small kernel asks for
    g = spectra.grid(64, 112)
    assert g.n == SMALL_MAX
    a = one(ops, g, max_iter=1024)
    b = one(ops, g, max_iter=1000)
    assert a[3]["small_segments"] == 1 and a[3]["large_segments"] == 0
    assert a[2] and a[1] < 1000
    assert a[:3] == b[:3]
    assert_exact(a[0], g.lam, "grid 64 x 112")
    # and with every slot of the tridiagonal scratch in use: a path that does not converge within 1,024 steps
    p = spectra.path(SMALL_MAX)
    lam, iters, conv, info = one(ops, p, max_iter=1024)
    assert iters == 1024 and not conv and info["not_converged"] == 1 and info["small_segments"] == 1
    lam0, iters0, _, _ = one(ops, p, max_iter=1000)
    assert iters0 == 1000 and lam0 < lam <= p.lam * (1 + 1e-14)


# ---------------------------------------------------------------------------------------------------- c. past the first chunk

GRIDS = [(85, 85), (100, 100), (60, 140)]


@pytest.mark.parametrize("ab", GRIDS, ids=lambda ab: f"{ab[0]}x{ab[1]}")
def test_past_first_chunk(ops, ab):
    g = spectra.grid(*ab)
    lam, iters, conv, info = one(ops, g)
    assert conv and iters > CHUNK, iters
    assert_exact(lam, g.lam, ab)
    assert_large_report(info, iters)
    assert info["not_converged"] == 0


def test_past_first_chunk_together(ops):
    gs = [spectra.grid(*ab) for ab in GRIDS]
    st, info = stats(ops, gs)
    alone = [one(ops, g) for g in gs]
    for s, g in enumerate(gs):
        assert (float(st["lambda_max"][s]), int(st["iters"][s]), bool(st["converged"][s])) == alone[s][:3], s
        assert_exact(float(st["lambda_max"][s]), g.lam, GRIDS[s])
    assert len(set(a[1] for a in alone)) == 3   # (three different stopping steps)
    assert_large_report(info, max(a[1] for a in alone), large=3)


# ---------------------------------------------------------------------------------------------------- d. segments stepping together

def mixed_segments():
    large = [spectra.cycle(8000), spectra.hypercube(13), spectra.star(8000), spectra.kary_tree(2, 12)] + [spectra.grid(*ab) for ab in GRIDS]
    small = [spectra.path(50), spectra.star(100), spectra.complete_bipartite(3, 5), spectra.grid(30, 40), spectra.wheel(500),
             spectra.torus(20, 30)]
    segs = large + small + [None, None, None]
    order = np.random.RandomState(7).permutation(len(segs))
    return [segs[i] for i in order], len(large), len(small)


def _check_mixed(ops, segs, nlarge, nsmall, node_ptr):
    st, info = stats(ops, segs, node_ptr=node_ptr)
    assert info["small_segments"] == nsmall and info["large_segments"] == nlarge, info
    most = 0
    for s, g in enumerate(segs):
        got = (float(st["lambda_max"][s]), int(st["iters"][s]), bool(st["converged"][s]))
        if g is None:
            assert got == (0.0, 0, True) and int(st["nodes"][s]) == 0, s
            continue
        assert int(st["nodes"][s]) == g.n, s
        alone = one(ops, g)
        assert got == alone[:3], (s, g.n, got, alone[:3])
        assert got[2], (s, g.n)
        assert_exact(got[0], g.lam, (s, g.n))
        most = max(most, got[1])
    assert info["lanczos_steps"] == most
    assert info["not_converged"] == 0
    large_most = max(int(st["iters"][s]) for s, g in enumerate(segs) if g is not None and g.n > SMALL_MAX)
    steps = CHUNK * math.ceil(large_most / CHUNK)
    assert info["large_steps"] == steps and info["large_launches"] == 4 * steps, info
    assert info["host_syncs"] == 3 + steps // CHUNK, info


def test_segments_step_together(ops):
    segs, nlarge, nsmall = mixed_segments()
    _check_mixed(ops, segs, nlarge, nsmall, None)


def test_segments_step_together_node_ptr(ops):
    segs, nlarge, nsmall = mixed_segments()
    G = len(segs) // 2   # (16 segments, 8 graphs: segments s and s + 8 share graph s's id range)
    assert 2 * G == len(segs)
    sizes = [max(g.n if g is not None else 0 for g in (segs[i], segs[i + G])) + 3 for i in range(G)]
    node_ptr = [0] + np.cumsum(sizes).tolist()
    _check_mixed(ops, segs, nlarge, nsmall, node_ptr)


def test_stopping_steps_are_spread(ops):
    # the large segments of the mixed call stop at very different steps: within the first check, near it, and several chunks on
    cyc = one(ops, spectra.cycle(8000))
    star = one(ops, spectra.star(8000))
    tree = one(ops, spectra.kary_tree(2, 12))
    grid = one(ops, spectra.grid(60, 140))
    assert cyc[1] <= 4 and star[1] <= 4 and tree[1] <= 16 and grid[1] > 4 * CHUNK, (cyc[1], star[1], tree[1], grid[1])


# ---------------------------------------------------------------------------------------------------- e. weights

def with_weights(g, w):
    sc = g.sc.copy()
    sc[:, 2] = w
    return spectra.Graph(sc, g.n, float("nan"))


def random_weights(g, seed):
    """Tie-free symmetric weights in [0.5, 1.5) for g's rows."""
    return sym_weights(g.sc[:, :2].T.astype(np.int64), g.n, seed)


@pytest.mark.parametrize("c", [0.3, 3.0])
def test_constant_weight_large(ops, c):
    g = spectra.scaled(spectra.grid(85, 85), c)
    lam, _, conv, info = one(ops, g, weighted=True)
    assert conv and info["large_segments"] == 1
    assert_exact(lam, g.lam, c)
    assert_exact(one(ops, g, weighted=False)[0], g.lam / c, c)


def weighted_lanczos_reference(sc, n, steps):
    """Largest eigenvalue of the weighted adjacency by Lanczos with full reorthogonalisation (torch float64, sparse A) from the
    normalised ones vector on the ids with a column."""
    r, c = sc[:, 0].long(), sc[:, 1].long()
    A = torch.sparse_coo_tensor(torch.stack([r, c]), sc[:, 2], (n, n)).coalesce().to_sparse_csr()
    ids = torch.unique(c)
    q = torch.zeros(n, dtype=torch.float64, device=sc.device)
    q[ids] = 1.0 / np.sqrt(ids.numel())
    V = [q]
    al, be = [], []
    for _ in range(steps):
        w = A @ V[-1]
        al.append(float(w @ V[-1]))
        Vm = torch.stack(V, 1)
        w = w - Vm @ (Vm.t() @ w)
        w = w - Vm @ (Vm.t() @ w)
        b = float(torch.linalg.norm(w))
        be.append(b)
        V.append(w / b)
    T = np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1)
    return float(np.linalg.eigvalsh(T)[-1])


@pytest.mark.parametrize("kind", ["sym", "wide6"])
def test_weighted_schur_snapshot_large(ops, kind):
    n = 20000
    ei_np = ba_graph(n, 5, 3)
    w_np = sym_weights(ei_np, n, 4) if kind == "sym" else wide_weights(ei_np, n, 5, 6)
    ei = torch.from_numpy(ei_np).cuda()
    sc = ops.approximate_cholesky(ei, torch.from_numpy(w_np).cuda(), n, n // 2, "random", "asc", seed=2, return_device="same")
    st = ops.snapshot_stats(sc, [0, sc.shape[0]], n, weighted=True)
    assert ops.last_stats["large_segments"] == 1
    assert bool(st["converged"][0])
    ref = weighted_lanczos_reference(sc, n, 120)
    assert_exact(float(st["lambda_max"][0]), ref, kind)
    unw = ops.snapshot_stats(sc, [0, sc.shape[0]], n)
    assert float(unw["lambda_max"][0]) != float(st["lambda_max"][0])


WEIGHTED = {
    "small_grid": lambda: spectra.grid(40, 50),
    "small_wheel": lambda: spectra.wheel(3000),
    "large_grid": lambda: spectra.grid(85, 85),
    "large_tree": lambda: spectra.kary_tree(3, 8),
}


@pytest.mark.parametrize("name", sorted(WEIGHTED))
def test_power_of_two_scaling(ops, name):
    g = WEIGHTED[name]()
    w = random_weights(g, 11)
    base = one(ops, with_weights(g, w), weighted=True)
    assert base[2]
    assert base[3]["large_segments"] == (1 if name.startswith("large") else 0)
    for e in (20, -20):
        got = one(ops, with_weights(g, w * 2.0 ** e), weighted=True)
        assert got[0] == base[0] * 2.0 ** e and got[1:3] == base[1:3], (e, got[:3], base[:3])


@pytest.mark.parametrize("name", sorted(WEIGHTED))
def test_unit_weights_weighted_equals_unweighted(ops, name):
    g = WEIGHTED[name]()
    a = one(ops, g, weighted=True)
    b = one(ops, g, weighted=False)
    assert a[:3] == b[:3]
    assert a[2]
    assert_exact(a[0], g.lam, name)


# ---------------------------------------------------------------------------------------------------- f. max_iter and tol

MAX_ITERS = [1, 2, 3, 4, 5, 31, 32, 33, 64, 1024]


def _max_iter_sweep(ops, g, large):
    prev = -math.inf
    for mi in MAX_ITERS:
        lam, iters, conv, info = one(ops, g, max_iter=mi)
        assert iters == mi and not conv, (mi, iters, conv)
        assert info["not_converged"] == 1 and info["lanczos_steps"] == mi, (mi, info)
        assert lam <= g.lam * (1 + 1e-14), (mi, lam, g.lam)   # (a Ritz value is a lower bound)
        assert lam >= prev, (mi, lam, prev)                    # (T_j's prefix does not depend on max_iter)
        prev = lam
        if large:
            assert info["large_segments"] == 1
            assert info["large_steps"] == mi and info["large_launches"] == 4 * mi, (mi, info)
            assert info["host_syncs"] == 3 + math.ceil(mi / CHUNK), (mi, info)
        else:
            assert info["small_segments"] == 1 and info["large_steps"] == 0, (mi, info)
    assert g.lam - prev < 1e-6


def test_max_iter_small(ops):
    _max_iter_sweep(ops, spectra.path(3000), False)


def test_max_iter_large(ops):
    _max_iter_sweep(ops, spectra.path(9000), True)
    info = one(ops, spectra.path(9000), max_iter=33)[3]
    assert info["large_steps"] == 33 and info["host_syncs"] == 5   # (chunks of 32 steps and 1 step)


@pytest.mark.parametrize("ab", [(85, 85), (60, 140), (64, 112)], ids=lambda ab: f"{ab[0]}x{ab[1]}")
def test_tol(ops, ab):
    g = spectra.grid(*ab)
    prev = None
    for tol in (1e-10, 1e-8, 1e-6, 1e-4):
        lam, iters, conv, info = one(ops, g, tol=tol)
        assert conv and info["not_converged"] == 0
        assert abs(lam - g.lam) <= tol * g.lam, (tol, lam, g.lam)
        assert lam <= g.lam * (1 + 1e-14)
        if prev is not None:
            assert iters <= prev, (tol, iters, prev)
        prev = iters


# ---------------------------------------------------------------------------------------------------- g. breakdowns, hidden components

@pytest.mark.parametrize("name", ["cycle_8000", "hypercube_13", "torus_90x91"])
def test_breakdown_large(ops, name):
    g = {"cycle_8000": lambda: spectra.cycle(8000), "hypercube_13": lambda: spectra.hypercube(13),
         "torus_90x91": lambda: spectra.torus(90, 91)}[name]()
    lam, iters, conv, info = one(ops, g)
    assert info["large_segments"] == 1
    assert conv and iters <= 4, iters
    assert_exact(lam, g.lam, name, rel=1e-14)
    assert_large_report(info, iters)


@pytest.mark.parametrize("k", [16, 25])
def test_hidden_component_large(ops, k):
    # a small component far off in the ids, whose lambda (4, then 5) is above the grid's 3.9973
    g = spectra.union(spectra.grid(85, 85), spectra.star(k))
    assert g.n > SMALL_MAX
    lam, iters, conv, info = one(ops, g)
    assert info["large_segments"] == 1
    assert conv
    assert_exact(lam, float(math.isqrt(k)), k)
    assert_large_report(info, iters)
    # the same component in front of the grid
    h = spectra.union(spectra.star(k), spectra.grid(85, 85))
    lam2, _, conv2, _ = one(ops, h)
    assert conv2
    assert_exact(lam2, float(math.isqrt(k)), k)
