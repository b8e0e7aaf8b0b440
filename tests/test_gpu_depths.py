"""Nested Schur complements (ops.approximate_cholesky_depths, rlap_approx_chol_depths): K depths of one graph from one elimination.

Contract (include/rlap_hip.h): snapshot k equals approximate_cholesky(..., num_remove=t_k) with the same perm / seed / mode -- indices,
row order and weights bit-exact -- and so the CPU oracle's single call at t_k.  Every call that is not meant to retry finishes in one
attempt (n_retries == 0) on the kernel it is pinned to."""
import os

import numpy as np
import pytest
import torch

import oracle
from util import assert_kernel, ba_graph, clique, default_kernel, grid2d, path, star, sym_weights, symmetrize, wide_weights

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::rlap_amd.ops.DataflowFallbackWarning")]

PAIRS = [(a, b) for a in ("random", "degree", "coarsen") for b in ("asc", "desc", "random")]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(params=["0", "1"])
def flow(request, monkeypatch):
    """RLAP_FLOW for the o_v = random calls: 0 the round kernel, 1 the dataflow kernel (the other orders always run the round kernel)."""
    monkeypatch.setenv("RLAP_FLOW", request.param)
    return int(request.param)


def expected_kernel(o_v, n):
    env = os.environ.get("RLAP_FLOW")
    if o_v == "random" and env is not None:
        return 2 if env == "1" else 1
    return default_kernel(o_v, 1, n)


def assert_same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: rows {a.shape} vs {b.shape}"
    assert np.array_equal(a[:, :2], b[:, :2]), f"{what}: indices differ"
    assert np.array_equal(a[:, 2], b[:, 2]), f"{what}: weights differ"


def depths(ops, ei, w, n, ts, o_v, o_n, *, perm=None, seed=7, mode="exact", retries_ok=False, kernel=None):
    ei_t = torch.from_numpy(np.ascontiguousarray(ei)).cuda()
    w_t = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64)).cuda()
    p_t = None if perm is None else torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int64))
    sc, ptr = ops.approximate_cholesky_depths(ei_t, w_t, n, ts, o_v, o_n, perm=p_t, seed=seed, mode=mode)
    st = ops.last_stats
    if not retries_ok:
        assert st["n_retries"] == 0, f"{o_v}/{o_n}: the call was repeated ({st})"
    assert st["n_eliminated"] == max(0, min(ts[-1], n - 1))
    if st["n_eliminated"] > 0:
        assert_kernel(ops, expected_kernel(o_v, n) if kernel is None else kernel, f"depths {o_v}/{o_n}")
    sc, ptr = sc.cpu().numpy(), ptr.numpy()
    assert len(ptr) == len(ts) + 1 and ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and ptr[-1] == sc.shape[0] == st["out_rows"]
    return [sc[int(ptr[k]):int(ptr[k + 1])] for k in range(len(ts))]


def single(ops, ei, w, n, t, o_v, o_n, *, perm=None, seed=7, mode="exact"):
    ei_t = torch.from_numpy(np.ascontiguousarray(ei)).cuda()
    w_t = None if w is None else torch.from_numpy(np.asarray(w, dtype=np.float64)).cuda()
    p_t = None if perm is None else torch.from_numpy(np.ascontiguousarray(perm, dtype=np.int64))
    a = ops.approximate_cholesky(ei_t, w_t, n, t, o_v, o_n, perm=p_t, seed=seed, mode=mode).numpy()
    assert ops.last_stats["n_retries"] == 0
    if min(t, n - 1) > 0:
        assert_kernel(ops, expected_kernel(o_v, n), f"single {o_v}/{o_n} t={t}")
    return a


def check_all(ops, ei, w, n, ts, o_v, o_n, what, *, perm=None, seed=7, mode="exact", gpu_single=True):
    snaps = depths(ops, ei, w, n, ts, o_v, o_n, perm=perm, seed=seed, mode=mode)
    for k, t in enumerate(ts):
        if not (o_v == "random" and perm is None):   # (a node_id vector drawn on the device: compared with the single GPU call only)
            ref = oracle.approximate_cholesky(ei, w, n, t, o_v, o_n, perm=perm, shuffle_seed=seed, mode=mode)
            assert_same(snaps[k], ref, f"{what} {o_v}/{o_n} snapshot {k} (t={t}) vs oracle")
        if gpu_single:
            assert_same(snaps[k], single(ops, ei, w, n, t, o_v, o_n, perm=perm, seed=seed, mode=mode), f"{what} {o_v}/{o_n} snapshot {k} vs single")
    return snaps


def graphs():
    """(name, edge_index, weights, n): small graphs of every shape the elimination meets."""
    out = []
    n = 500
    ei = ba_graph(n, 5, 3)
    out.append(("ba500", ei, None, n))
    out.append(("ba500-sym", ei, sym_weights(ei, n, 4), n))
    out.append(("ba500-wide", ei, wide_weights(ei, n, 5, 6), n))
    out.append(("clique24", clique(24), None, 24))
    out.append(("star60", star(60), None, 60))
    out.append(("path80", path(80), None, 80))
    out.append(("grid12x13", grid2d(12, 13), None, 156))
    iso = ba_graph(200, 3, 6)
    out.append(("isolated-tail", iso, None, 230))   # vertices 200..229 have no edge
    return out


@pytest.mark.parametrize("name,ei,w,n", graphs(), ids=[g[0] for g in graphs()])
def test_every_pair_matches_oracle_and_single_calls(ops, flow, name, ei, w, n):
    ts = [0, n // 8, n // 4, n // 4, n // 2, n - 1, n + 5]
    perm = np.random.RandomState(2).permutation(n)
    for o_v, o_n in PAIRS:
        if flow == 1 and o_v != "random":
            continue   # (the round kernel's orders run once, under RLAP_FLOW=0)
        check_all(ops, ei, w, n, ts, o_v, o_n, name, perm=perm if o_v == "random" else None, seed=11)


def test_duplicate_and_unsorted_input(ops, flow):
    n = 400
    ei = ba_graph(n, 4, 8)
    rng = np.random.RandomState(3)
    w = sym_weights(ei, n, 9)
    order = rng.permutation(ei.shape[1])
    eu, wu = ei[:, order], w[order]                                      # unsorted
    sel = np.arange(0, 300)
    ed = np.concatenate([ei, ei[:, sel], ei[::-1, sel]], axis=1)         # duplicated edges, both directions (summed, like the single call)
    wd = np.concatenate([w, w[sel], w[sel]])
    ts = [n // 8, n // 3, n // 2]
    for o_v, o_n in (("random", "asc"), ("degree", "random"), ("coarsen", "desc")):
        if flow == 1 and o_v != "random":
            continue
        perm = np.random.RandomState(4).permutation(n) if o_v == "random" else None
        check_all(ops, eu, wu, n, ts, o_v, o_n, "unsorted", perm=perm, seed=5)
        check_all(ops, ed, wd, n, ts, o_v, o_n, "duplicates", perm=perm, seed=5)


def test_large_ba_many_positions_in_flight(ops, flow):
    """BA(120000, 4): the dataflow kernel has thousands of positions in flight when a segment stops and the next one starts."""
    n = 120000
    ei = ba_graph(n, 4, 21)
    ts = [n // 8, n // 4, n // 2]
    perm = np.random.RandomState(22).permutation(n)
    check_all(ops, ei, None, n, ts, "random", "asc", "ba120k", perm=perm, seed=3, gpu_single=False)
    if flow == 0:
        check_all(ops, ei, None, n, ts, "degree", "asc", "ba120k", seed=3, gpu_single=False)


def test_k1_equals_single_and_k8(ops):
    n = 1500
    ei = ba_graph(n, 6, 31)
    for o_v, o_n in (("random", "asc"), ("degree", "asc"), ("coarsen", "random")):
        for t in (0, n // 3, n):
            snaps = depths(ops, ei, None, n, [t], o_v, o_n, seed=4)
            assert_same(snaps[0], single(ops, ei, None, n, t, o_v, o_n, seed=4), f"K=1 {o_v}/{o_n} t={t}")
        ts = sorted(np.random.RandomState(5).randint(0, n, size=8).tolist())
        check_all(ops, ei, None, n, ts, o_v, o_n, "K=8", seed=4)


def test_perm_seeds_and_frontier(ops, flow):
    n = 2000
    ei = ba_graph(n, 5, 41)
    ts = [n // 8, n // 4, n // 2]
    for s in (0, 1, 12345):
        perm = np.random.RandomState(s).permutation(n)
        check_all(ops, ei, None, n, ts, "random", "random", f"perm seed {s}", perm=perm, seed=s)
        check_all(ops, ei, None, n, ts, "random", "asc", f"drawn perm seed {s}", seed=s)   # the node_id vector drawn from the seed
    for o_v, o_n in (("random", "asc"), ("degree", "random"), ("coarsen", "asc")):
        if flow == 1 and o_v != "random":
            continue
        check_all(ops, ei, None, n, ts, o_v, o_n, "frontier", seed=9, mode="frontier")


def test_poison_and_jitter(ops, flow):
    n = 3000
    ei = ba_graph(n, 6, 9)
    ts = [n // 8, n // 4, n // 2]
    perm = np.random.RandomState(8).permutation(n)
    cases = [("random", "asc")] + ([("degree", "asc"), ("coarsen", "random")] if flow == 0 else [])
    base = {c: depths(ops, ei, None, n, ts, *c, perm=perm if c[0] == "random" else None, seed=3) for c in cases}
    ops.debug_set_poison(0xA5)
    ops.debug_set_jitter(8)
    try:
        for c in cases:
            got = depths(ops, ei, None, n, ts, *c, perm=perm if c[0] == "random" else None, seed=3)
            for k in range(len(ts)):
                assert_same(got[k], base[c][k], f"poison + jitter {c} snapshot {k}")
    finally:
        ops.debug_set_poison(-1)
        ops.debug_set_jitter(0)


def test_growth_retry_in_a_later_segment(ops, flow):
    """A uniform table that holds the first snapshot's draws and no more: the overflow strikes in the second of three segments, the
    third one (behind a failed segment) eliminates nothing, the whole call is repeated from depth 0 (retry kind 3) and every
    snapshot is still exact."""
    from rlap_amd import _lib
    n = 3000
    ei = ba_graph(n, 6, 19)
    ts = [n // 8, n // 4, n // 2]
    perm = np.random.RandomState(18).permutation(n)
    for o_v, o_n in (("random", "asc"), ("degree", "asc")):
        if flow == 1 and o_v != "random":
            continue
        p = perm if o_v == "random" else None
        base = depths(ops, ei, None, n, ts, o_v, o_n, perm=p, seed=3)
        single(ops, ei, None, n, ts[0], o_v, o_n, perm=p, seed=3)
        d0 = ops.last_stats["n_draws"]
        single(ops, ei, None, n, ts[-1], o_v, o_n, perm=p, seed=3)
        assert ops.last_stats["n_draws"] > d0 + 4096
        ops.debug_set_limits(rng_len=d0 + 64)
        try:
            got = depths(ops, ei, None, n, ts, o_v, o_n, perm=p, seed=3, retries_ok=True)
            st = ops.last_stats
        finally:
            ops.debug_set_limits()
        assert st["n_retries"] == 1 and st["retry_causes"] == _lib.RETRY_RNG, st
        for k in range(len(ts)):
            assert_same(got[k], base[k], f"rng retry {o_v} snapshot {k}")
            assert_same(got[k], oracle.approximate_cholesky(ei, None, n, ts[k], o_v, o_n, perm=p, shuffle_seed=3), f"rng retry {o_v} oracle {k}")


def test_reorder_fallback_moves_the_call_to_the_round_kernel(ops, monkeypatch):
    """Two hubs that collect thousands of out-of-order appended entries and survive every depth, with a reorder buffer of one entry
    (rlap_debug_set_flow_limits): the tag-order pass of the first snapshot cannot hold them (retry kind 7, quiet), the whole call
    moves to the round kernel, and every snapshot is the oracle's."""
    from rlap_amd import _lib
    monkeypatch.setenv("RLAP_FLOW", "1")
    rng = np.random.RandomState(12)
    n = 3000
    a0 = np.concatenate([np.zeros(n - 2, dtype=np.int64), np.ones(n - 2, dtype=np.int64), np.arange(2, n - 1)])
    b0 = np.concatenate([np.arange(2, n), np.arange(2, n), np.arange(3, n)])
    ei = symmetrize(a0, b0, n)
    perm = np.concatenate([[0, 1], 2 + rng.permutation(n - 2)])   # the hubs go last
    ts = [n // 4, n // 2, n - 3]
    ops.debug_set_flow_limits(1)
    got = depths(ops, ei, None, n, ts, "random", "asc", perm=perm, seed=3, retries_ok=True, kernel=_lib.KERNEL_ROUND)
    st = ops.last_stats
    assert st["retry_causes"] == _lib.RETRY_FLOW_REORDER and st["flow_abort"] == 0 and st["n_retries"] == 1, st
    for k, t in enumerate(ts):
        assert_same(got[k], oracle.approximate_cholesky(ei, None, n, t, "random", "asc", perm=perm, shuffle_seed=3), f"fallback snapshot {k}")
    got2 = depths(ops, ei, None, n, ts, "random", "asc", perm=perm, seed=3)   # (the limit held for one attempt only)
    for k in range(len(ts)):
        assert_same(got2[k], got[k], f"dataflow again, snapshot {k}")


def test_bad_arguments_of_the_c_abi(ops):
    from rlap_amd import _lib
    lib = _lib.load()
    n = 50
    ei = torch.from_numpy(path(n)).cuda()
    row, col = ei[0].contiguous(), ei[1].contiguous()
    out = torch.empty((3 * ei.shape[1], 3), dtype=torch.float64, device="cuda")
    ptr = torch.zeros(4, dtype=torch.int64)
    h = ops._handle(ei.device)[1]
    for ts, K in (([5, 3, 9], 3), ([1, 2, 3], 0)):
        t = torch.tensor(ts, dtype=torch.int64)
        assert lib.rlap_approx_chol_depths(h, row.data_ptr(), col.data_ptr(), None, ei.shape[1], n, K, t.data_ptr(), 1, 0, None, 0,
                                           out.data_ptr(), out.shape[0], ptr.data_ptr(), None) == 3, (ts, K)
    assert lib.rlap_approx_chol_depths(h, row.data_ptr(), col.data_ptr(), None, ei.shape[1], n, 3, None, 1, 0, None, 0,
                                       out.data_ptr(), out.shape[0], ptr.data_ptr(), None) == 3
    assert lib.rlap_approx_chol_depths(None, None, None, None, 0, 1, 1, None, 0, 0, None, 0, None, 0, None, None) == 3


def test_adapter_depths(ops):
    from rlap_amd import adapters
    n = 1500
    ei = torch.from_numpy(ba_graph(n, 5, 2)).cuda()
    x = torch.zeros(n, 4, device="cuda")
    gs = adapters.rLapDepths(fracs=(0.1, 0.3, 0.6), o_v="degree", o_n="asc", keep_weights=True).augment((x, ei, None))
    assert ops.last_stats["n_retries"] == 0
    assert_kernel(ops, expected_kernel("degree", n), "rLapDepths")
    for f, g in zip((0.1, 0.3, 0.6), gs):
        a = ops.approximate_cholesky(ei, None, n, int(f * n), "degree", "asc", return_device="same")
        assert ops.last_stats["n_retries"] == 0
        assert_kernel(ops, expected_kernel("degree", n), f"single degree/asc at {f}")
        assert torch.equal(g.edge_index, a[:, :2].long().t()) and torch.equal(g.edge_weights, a[:, 2])
