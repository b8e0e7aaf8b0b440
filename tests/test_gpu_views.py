"""Multi-view Schur complements (ops.approximate_cholesky_views, rlap_approx_chol_views): K views of one input in one call.

Contract (include/rlap_hip.h): (view k, graph g) equals graph k*G + g of approximate_cholesky_batched on the K-fold disjoint union of
the input, with the same seed, ids shifted back -- i.e. a single call on graph g with seed + k*G + g and perm slice (k, g).  Bar:
indices, row order and weights bit-exact.  Every call but the ones that force a retry must finish in one attempt (n_retries == 0), so
that a silent fall-back of the dataflow kernel to the round kernel cannot pass unseen."""
import numpy as np
import pytest
import torch

import os

import oracle
from util import assert_kernel, ba_graph, clique, default_kernel, sym_weights, wide_weights

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::rlap_amd.ops.DataflowFallbackWarning")]

PAIRS = [(a, b) for a in ("random", "degree", "coarsen") for b in ("asc", "desc", "random")]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def assert_same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: rows {a.shape} vs {b.shape}"
    assert np.array_equal(a[:, :2], b[:, :2]), f"{what}: indices differ"
    assert np.array_equal(a[:, 2], b[:, 2]), f"{what}: weights differ"


def views(ops, ei, w, n, ts, o_v, o_n, *, node_ptr=None, perm=None, seed=7, mode="exact", retries_ok=False, kernel=None):
    """One views call; `kernel`: the elim_kernel expected (None: the default rule's choice for the K * G graphs of the union, unless
    RLAP_FLOW overrides it)."""
    ei_t = torch.from_numpy(np.ascontiguousarray(ei)).cuda()
    w_t = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64)).cuda()
    p_t = None if perm is None else torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int64))
    sc, ptr = ops.approximate_cholesky_views(ei_t, w_t, n, ts, o_v, o_n, node_ptr=node_ptr, perm=p_t, seed=seed, mode=mode)
    if not retries_ok:
        assert ops.last_stats["n_retries"] == 0, f"{o_v}/{o_n}: the call was repeated ({ops.last_stats})"
    if kernel is None and os.environ.get("RLAP_FLOW") is None:
        kernel = default_kernel(o_v, len(ptr) - 1, (len(ptr) - 1) // (1 if node_ptr is None else len(node_ptr) - 1) * n)
    if kernel is not None and ops.last_stats["n_eliminated"] > 0:
        assert_kernel(ops, kernel, f"views {o_v}/{o_n}")
    return sc.cpu().numpy(), ptr.numpy()


def split(sc, ptr):
    return [sc[int(ptr[i]):int(ptr[i + 1])] for i in range(len(ptr) - 1)]


def perms_for(K, n, seed=0):
    return [np.random.RandomState(seed + k).permutation(n) for k in range(K)]


def check_symmetric(v, n, what):
    if v.shape[0] == 0:
        return
    assert v[:, :2].min() >= 0 and v[:, :2].max() < n, f"{what}: ids outside [0, {n})"
    fw = set(map(tuple, v[:, :2].astype(np.int64).tolist()))   # (the edge pattern: rows may repeat a pair, as multi-edges)
    assert all((c, r) in fw for r, c in fw), f"{what}: not symmetric"


@pytest.mark.parametrize("graph", ["ba", "clique"])
def test_one_view_equals_approximate_cholesky(ops, graph):
    n = 400 if graph == "ba" else 24
    ei = ba_graph(n, 5, 3) if graph == "ba" else clique(n)
    ei_t = torch.from_numpy(ei).cuda()
    perm = np.random.RandomState(1).permutation(n)
    for o_v, o_n in PAIRS:
        p = torch.from_numpy(perm) if o_v == "random" else None
        a = ops.approximate_cholesky(ei_t, None, n, n // 2, o_v, o_n, perm=p, seed=11).numpy()
        b, ptr = views(ops, ei, None, n, n // 2, o_v, o_n, perm=perm if o_v == "random" else None, seed=11)
        assert list(ptr) == [0, a.shape[0]]
        assert_same(b, a, f"K=1 {graph} {o_v}/{o_n}")
        # ... also without an injected perm: the same keyed draw from the seed
        if o_v == "random":
            a = ops.approximate_cholesky(ei_t, None, n, n // 2, o_v, o_n, seed=11).numpy()
            b, _ = views(ops, ei, None, n, [n // 2], o_v, o_n, seed=11)
            assert_same(b, a, f"K=1 {graph} {o_v}/{o_n}, drawn perm")


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("o_v,o_n", PAIRS)
def test_every_view_equals_the_oracle(ops, K, o_v, o_n):
    n = 300
    ei = ba_graph(n, 4, 17)
    choices = [0, 1, n // 2, n - 1, n + 3]
    for shift in (0, 2):
        ts = [choices[(k + shift) % len(choices)] for k in range(K)]
        perms = perms_for(K, n, 3 * K + shift)
        sc, ptr = views(ops, ei, None, n, ts, o_v, o_n, perm=np.concatenate(perms) if o_v == "random" else None, seed=40)
        assert len(ptr) == K + 1 and ptr[0] == 0 and ptr[-1] == sc.shape[0]
        for k, v in enumerate(split(sc, ptr)):
            ref = oracle.approximate_cholesky(ei, None, n, ts[k], o_v, o_n, perm=perms[k] if o_v == "random" else None, shuffle_seed=40 + k)
            assert_same(v, ref, f"K={K} view {k} t={ts[k]} {o_v}/{o_n}")
            check_symmetric(v, n, f"view {k}")


def union_reference(ops, ei, w, n, K, ts, o_v, o_n, perm, seed):
    from rlap_amd import graphs
    big, node_ptr = graphs.batch_disjoint([torch.from_numpy(ei)] * K, [n] * K)
    w_t = None if w is None else torch.from_numpy(np.tile(np.asarray(w, dtype=np.float64), K)).cuda()
    p_t = None if perm is None else torch.from_numpy(perm)
    sc, rp = ops.approximate_cholesky_batched(big.cuda(), w_t, node_ptr, ts, o_v, o_n, perm=p_t, seed=seed)
    assert ops.last_stats["n_retries"] == 0
    out = []
    for k, v in enumerate(split(sc.cpu().numpy(), rp.numpy())):
        v = v.copy()
        v[:, :2] -= k * n
        out.append(v)
    return out


@pytest.mark.parametrize("flow", ["default", "0"])
def test_views_equal_the_batched_union_random_order(ops, monkeypatch, flow):
    """o_v = random on BA(20000, 5), K = 2: the dataflow kernel is chosen by default (a pair of graphs); RLAP_FLOW=0 the round kernel.
    Unit weights, and log-uniform weights over 10^+-30 (the dead-entry rules)."""
    kernel = 2 if flow == "default" else 1
    if flow == "0":
        monkeypatch.setenv("RLAP_FLOW", "0")
    n, K = 20000, 2
    ei = ba_graph(n, 5, 21)
    ts = [n // 2, n // 3]
    given = np.concatenate(perms_for(K, n, 5))
    for perm, w in ((None, None), (given, wide_weights(ei, n, 8, 30)), (given, None)):
        got, ptr = views(ops, ei, w, n, ts, "random", "asc", perm=perm, seed=123, kernel=kernel)
        ref = union_reference(ops, ei, w, n, K, ts, "random", "asc", perm, 123)
        assert_kernel(ops, kernel, f"the batched union, flow={flow}")
        for k, v in enumerate(split(got, ptr)):
            assert_same(v, ref[k], f"view {k} flow={flow} perm={'given' if perm is not None else 'drawn'} weighted={w is not None}")
    # one view against the oracle at this size too
    perms = perms_for(K, n, 5)
    a = oracle.approximate_cholesky(ei, None, n, ts[1], "random", "asc", perm=perms[1], shuffle_seed=124)
    assert_same(split(got, ptr)[1], a, "view 1 vs oracle")


@pytest.mark.parametrize("o_v,o_n", [("degree", "asc"), ("degree", "random"), ("coarsen", "asc"), ("coarsen", "random")])
def test_views_equal_the_batched_union_round_kernel(ops, o_v, o_n):
    n, K = 5000, 3
    ei = ba_graph(n, 6, 8)
    w = sym_weights(ei, n, 4)
    ts = [n // 2, n // 4, n // 2]
    got, ptr = views(ops, ei, w, n, ts, o_v, o_n, seed=99)
    ref = union_reference(ops, ei, w, n, K, ts, o_v, o_n, None, 99)
    for k, v in enumerate(split(got, ptr)):
        assert_same(v, ref[k], f"view {k} {o_v}/{o_n}")


@pytest.mark.parametrize("o_v,o_n", [("degree", "asc"), ("random", "asc"), ("coarsen", "random"), ("random", "random")])
def test_batched_input_times_views(ops, o_v, o_n):
    """G = 4 graphs of different sizes, K = 2: (view k, graph g) is a single call on graph g with seed + k*G + g, rows view-major."""
    from rlap_amd import graphs
    ns = [50, 333, 7, 1200]
    eis = [ba_graph(m, 3, 60 + g) for g, m in enumerate(ns)]
    big, node_ptr = graphs.batch_disjoint([torch.from_numpy(e) for e in eis], ns)
    G, K, N = len(ns), 2, sum(ns)
    ts = np.array([[m // 2 for m in ns], [m - 1 for m in ns]], dtype=np.int64)
    perms = [[np.random.RandomState(10 * k + g).permutation(m) for g, m in enumerate(ns)] for k in range(K)]
    perm = np.concatenate([np.concatenate(p) for p in perms]) if o_v == "random" else None
    sc, ptr = views(ops, big.numpy(), None, N, torch.from_numpy(ts), o_v, o_n, node_ptr=node_ptr, perm=perm, seed=1000)
    assert len(ptr) == K * G + 1 and ptr[-1] == sc.shape[0]
    for k in range(K):
        for g in range(G):
            v = sc[ptr[k * G + g]:ptr[k * G + g + 1]].copy()
            off = int(node_ptr[g])
            if v.shape[0]:
                assert v[:, :2].min() >= off and v[:, :2].max() < off + ns[g], f"view {k} graph {g}: ids outside the input's range"
            v[:, :2] -= off
            ref = oracle.approximate_cholesky(eis[g], None, ns[g], int(ts[k, g]), o_v, o_n,
                                              perm=perms[k][g] if o_v == "random" else None, shuffle_seed=1000 + k * G + g)
            assert_same(v, ref, f"view {k} graph {g} {o_v}/{o_n}")


@pytest.mark.parametrize("o_v", ["random", "degree"])
def test_frontier_mode(ops, o_v):
    n, K = 2000, 2
    ei = ba_graph(n, 5, 31)
    perms = perms_for(K, n, 2)
    perm = np.concatenate(perms) if o_v == "random" else None
    sc, ptr = views(ops, ei, None, n, [n // 2] * K, o_v, "asc", perm=perm, seed=77, mode="frontier")
    vs = split(sc, ptr)
    for k, v in enumerate(vs):
        ref = oracle.approximate_cholesky(ei, None, n, n // 2, o_v, "asc", perm=perms[k] if o_v == "random" else None,
                                          shuffle_seed=77 + k, mode="frontier")
        assert_same(v, ref, f"frontier view {k} {o_v}")
    assert not (vs[0].shape == vs[1].shape and np.array_equal(vs[0], vs[1])), "frontier: two views with equal t are identical"


def test_exact_degree_order_views_with_equal_t_are_identical(ops):
    """The reference's behaviour, documented: o_v = degree with o_n = asc draws from a default-seeded stream -- nothing per call."""
    n = 2000
    ei = ba_graph(n, 5, 31)
    sc, ptr = views(ops, ei, None, n, [n // 2, n // 2], "degree", "asc", seed=77)
    a, b = split(sc, ptr)
    assert a.shape[0] > 0
    assert_same(a, b, "degree/asc views with equal t")


def test_input_handling(ops, monkeypatch):
    n, K = 3000, 2
    ei = ba_graph(n, 6, 9)
    w = sym_weights(ei, n, 3)
    ts = [n // 2, n // 3]
    # weighted input
    for o_v, o_n in (("degree", "asc"), ("random", "random")):
        perms = perms_for(K, n, 1)
        sc, ptr = views(ops, ei, w, n, ts, o_v, o_n, perm=np.concatenate(perms) if o_v == "random" else None, seed=5)
        for k, v in enumerate(split(sc, ptr)):
            assert_same(v, oracle.approximate_cholesky(ei, w, n, ts[k], o_v, o_n, perm=perms[k] if o_v == "random" else None,
                                                       shuffle_seed=5 + k), f"weighted view {k} {o_v}/{o_n}")
    # unsorted columns, duplicate entries (both directions) and zero weights
    rs = np.random.RandomState(4)
    a, b = ei[0, :40], ei[1, :40]
    eid = np.concatenate([ei, np.stack([a, b]), np.stack([b, a])], axis=1)
    wd = np.concatenate([w, w[:40] * 0.5, w[:40] * 0.5])
    z = rs.choice(ei.shape[1], 30, replace=False)
    zero_pairs = set(zip(ei[0, z], ei[1, z])) | set(zip(ei[1, z], ei[0, z]))
    wd[[i for i in range(ei.shape[1]) if (ei[0, i], ei[1, i]) in zero_pairs]] = 0.0
    order = rs.permutation(eid.shape[1])
    eid, wd = eid[:, order], wd[order]
    sc, ptr = views(ops, eid, wd, n, ts, "degree", "random", seed=6)
    assert ops.last_stats["reserved"] == 0
    for k, v in enumerate(split(sc, ptr)):
        assert_same(v, oracle.approximate_cholesky(eid, wd, n, ts[k], "degree", "random", shuffle_seed=6 + k), f"dup/zero view {k}")
    # above the sort-skip threshold: an input in (row, col) order is read transposed, the sort skipped once for all views
    monkeypatch.setenv("RLAP_SORT_SKIP_MIN", "1")
    rc = np.lexsort((ei[1], ei[0]))
    sc, ptr = views(ops, ei[:, rc], w[rc], n, ts, "coarsen", "asc", seed=8)
    assert ops.last_stats["reserved"] == 2
    for k, v in enumerate(split(sc, ptr)):
        assert_same(v, oracle.approximate_cholesky(ei, w, n, ts[k], "coarsen", "asc", shuffle_seed=8 + k), f"(row,col)-sorted view {k}")
    monkeypatch.delenv("RLAP_SORT_SKIP_MIN")
    # asymmetric input: ValueError, and the handle still works afterwards
    w_bad = w.copy()
    w_bad[0] += 1.0
    with pytest.raises(ValueError):
        views(ops, ei, w_bad, n, ts, "degree", "asc")
    with pytest.raises(ValueError):
        views(ops, ei[:, 1:], None, n, ts, "random", "asc")
    sc, ptr = views(ops, ei, None, n, ts, "degree", "asc")
    assert_same(split(sc, ptr)[1], oracle.approximate_cholesky(ei, None, n, ts[1], "degree", "asc"), "after the rejected inputs")


def test_bad_arguments(ops):
    n = 100
    ei = torch.from_numpy(ba_graph(n, 3, 1)).cuda()
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_views(ei, None, n, [], "degree", "asc")   # K = 0
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_views(ei, None, n, [10, 10], "random", "asc", perm=torch.arange(n))   # perm needs K * n entries
    from rlap_amd import _lib
    lib = _lib.load()
    assert lib.rlap_approx_chol_views(None, None, None, None, 0, 1, None, 0, None, 0, 0, None, 0, None, 0, None, None) == 3


def test_poison_jitter_and_retry(ops):
    n, K = 3000, 2
    ei = ba_graph(n, 6, 9)
    ts = [n // 2, n // 4]
    perm = np.concatenate(perms_for(K, n, 8))
    base = {}
    for o_v in ("degree", "random"):
        base[o_v] = views(ops, ei, None, n, ts, o_v, "asc", perm=perm if o_v == "random" else None, seed=3)
    ops.debug_set_poison(0xA5)
    ops.debug_set_jitter(8)
    try:
        for o_v in ("degree", "random"):
            sc, ptr = views(ops, ei, None, n, ts, o_v, "asc", perm=perm if o_v == "random" else None, seed=3)
            assert_same(sc, base[o_v][0], f"poison + jitter {o_v}")
            assert np.array_equal(ptr, base[o_v][1])
    finally:
        ops.debug_set_poison(-1)
        ops.debug_set_jitter(0)
    for o_v, lim in (("degree", dict(pool_factor=0.0)), ("degree", dict(log_factor=0.0)), ("random", dict(rng_len=100)),
                     ("random", dict(pool_factor=0.0))):
        ops.debug_set_limits(**lim)
        try:
            sc, ptr = views(ops, ei, None, n, ts, o_v, "asc", perm=perm if o_v == "random" else None, seed=3, retries_ok=True)
            retries = ops.last_stats["n_retries"]
        finally:
            ops.debug_set_limits()
        assert retries > 0, f"{o_v} {lim}: the limit was not hit"
        assert_same(sc, base[o_v][0], f"retry {o_v} {lim}")


def test_adapter_views(ops):
    from rlap_amd import adapters
    n = 1500
    ei = torch.from_numpy(ba_graph(n, 5, 2)).cuda()
    x = torch.zeros(n, 4, device="cuda")
    aug = adapters.rLapViews(fracs=(0.3, 0.6), o_v="degree", o_n="asc", keep_weights=True)
    g1, g2 = aug.augment((x, ei, None))
    sc, ptr = ops.approximate_cholesky_views(ei, None, n, [int(0.3 * n), int(0.6 * n)], "degree", "asc")
    for k, g in enumerate((g1, g2)):
        part = sc[int(ptr[k]):int(ptr[k + 1])].cuda()
        assert torch.equal(g.edge_index, part[:, :2].long().t()) and torch.equal(g.edge_weights, part[:, 2])
    a1, a2 = adapters.rLapViews(fracs=(0.3, 0.6), o_v="degree", o_n="asc").augmentors()
    h1, h2 = a1(x, ei), a2(x, ei)
    assert torch.equal(h1.edge_index, g1.edge_index) and torch.equal(h2.edge_index, g2.edge_index)
    assert h1.edge_weights is None
