"""The degree order's two round kernels: 16-slot candidates first (256 per round, k_eliminate_batch_t<OV_DEGREE, *, 16, 1024>), then,
from the first column longer than 16 slots on, the 32-slot kernel launched behind it on the same stream (GraphDesc::resume).

Every case is bit-exact against the CPU oracle; rlap_stats.n_rounds_narrow (the part of n_rounds the 16-slot kernel ran) tells
whether, and how far, the 16-slot kernel ran."""
import numpy as np
import pytest
import torch

import oracle
from rlap_amd import _lib
from util import assert_kernel, ba_graph, grid2d, path, sym_weights
from test_gpu_parity import assert_same, gpu_call, _where

pytestmark = [pytest.mark.gpu]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def call(ops, ei, w, n, t, o_n, seed=9):
    """One degree-order call checked against the oracle; returns (rows, stats)."""
    got = gpu_call(ops, ei, w, n, t, "degree", o_n, seed=seed, kernel=_lib.KERNEL_ROUND)
    st = dict(ops.last_stats)
    assert st["n_retries"] == 0, st
    ref = oracle.approximate_cholesky(ei, w, n, t, "degree", o_n, shuffle_seed=seed)
    assert_same(got, ref, f"n={n} t={t} degree/{o_n}")
    print(f"n={n} t={t} degree/{o_n}: n_rounds {st['n_rounds']} n_rounds_narrow {st['n_rounds_narrow']} n_singles {st['n_singles']}")
    return got, st


@pytest.mark.parametrize("name", ["path", "grid", "ba_quarter"])
def test_graph_that_stays_narrow_to_the_end(ops, name):
    """No column at the head of the queue ever exceeds 16 slots: the 16-slot kernel runs every round and the 32-slot kernel behind
    it finds n_elim where it should stop."""
    if name == "path":
        n = 5000; ei = path(n); t = n - 1
    elif name == "grid":
        n = 64 * 64; ei = grid2d(64, 64); t = n // 3
    else:
        n = 8000; ei = ba_graph(n, 5, 4); t = n // 4
    _, st = call(ops, ei, None, n, t, "asc")
    assert st["n_rounds"] > 0 and st["n_rounds_narrow"] == st["n_rounds"], st


@pytest.mark.parametrize("o_n", ["asc", "desc", "random"])
@pytest.mark.parametrize("weights", ["unit", "tie_free"])
def test_hand_over_midway(ops, o_n, weights):
    """BA(n, 10), t = n/2: the columns at the head of the queue outgrow 16 slots on the way (tests/tools/round_stats.py)."""
    n = 20000
    ei = ba_graph(n, 10, 1)
    w = None if weights == "unit" else sym_weights(ei, n, 5)
    _, st = call(ops, ei, w, n, n // 2, o_n)
    assert 0 < st["n_rounds_narrow"] < st["n_rounds"], st


@pytest.mark.parametrize("o_n", ["asc", "random"])
def test_first_candidate_already_wide(ops, o_n):
    """BA(n, 20): the lowest degree is 20, so the 16-slot kernel stops in front of its first round."""
    n = 3000
    _, st = call(ops, ba_graph(n, 20, 2), None, n, n // 2, o_n)
    assert st["n_rounds_narrow"] == 0 and st["n_rounds"] > 0, st


def test_num_remove_limits(ops):
    n = 2000
    ei = ba_graph(n, 10, 3)
    for t in (0, 1, n - 1, n + 5):
        _, st = call(ops, ei, None, n, t, "asc")
        if t == 0:
            assert st["n_rounds"] == 0 and st["n_rounds_narrow"] == 0, st
        if t == 1:   # (lowest degree 10: the one vertex goes in one round of the 16-slot kernel)
            assert st["n_rounds"] == 1 and st["n_rounds_narrow"] == 1 and st["n_singles"] == 0, st


def test_batch_of_graphs_that_hand_over_at_different_points(ops):
    """Five graphs in one call (one workgroup each): one stays narrow, one is wide from the start, the others hand over at their
    own points.  Graph g equals a separate call on it with seed + g."""
    from rlap_amd import graphs
    spec = [(6000, 3), (5000, 10), (3000, 20), (9000, 8), (4000, 12)]
    eis = [ba_graph(n, m, 50 + g) for g, (n, m) in enumerate(spec)]
    ns = [n for n, _ in spec]
    ts = [n // 2 for n in ns]
    big, node_ptr = graphs.batch_disjoint([torch.from_numpy(e) for e in eis], ns)
    for o_n in ("asc", "desc"):
        sc, row_ptr = ops.approximate_cholesky_batched(big.cuda(), None, node_ptr, ts, "degree", o_n, seed=5)
        st = dict(ops.last_stats)
        assert_kernel(ops, _lib.KERNEL_ROUND, f"batch degree/{o_n}")
        assert st["n_retries"] == 0 and 0 < st["n_rounds_narrow"] < st["n_rounds"], st
        sc = sc.cpu().numpy()
        narrow_each = []
        for g, (n, m) in enumerate(spec):
            ref = oracle.approximate_cholesky(eis[g], None, n, ts[g], "degree", o_n, shuffle_seed=5 + g)
            b = sc[int(row_ptr[g]):int(row_ptr[g + 1])].copy()
            b[:, :2] -= int(node_ptr[g])
            assert_same(b, ref, f"graph {g} BA({n},{m}) degree/{o_n}")
            _, sg = call(ops, eis[g], None, n, ts[g], o_n, seed=5 + g)
            narrow_each.append(sg["n_rounds_narrow"])
        # the 16-slot kernel ends its rounds by rules that depend on the graph alone (contended records are placed in candidate
        # order), so a graph runs the same narrow rounds in the batch as in a call of its own
        assert sum(narrow_each) == st["n_rounds_narrow"], (narrow_each, st)
        assert narrow_each[2] == 0 and min(narrow_each[0], narrow_each[1], narrow_each[3]) > 0, narrow_each


@pytest.mark.parametrize("o_n", ["asc", "random"])
def test_depths_call_across_the_hand_over(ops, o_n):
    """Segments of a depths call launch the pair of kernels each: boundaries before the hand-over (the 16-slot kernel resumes), at
    a point behind it (later segments skip the 16-slot kernel) -- every snapshot equals the oracle's single call at its depth."""
    n = 20000
    ei = ba_graph(n, 10, 1)
    _, st_full = call(ops, ei, None, n, (3 * n) // 4, o_n, seed=7)
    assert 0 < st_full["n_rounds_narrow"] < st_full["n_rounds"], st_full
    ts = [n // 20, n // 5, n // 3, n // 2, (5 * n) // 8, (3 * n) // 4]
    # where the hand-over falls among the depths: a single call that stops at depth t in front of it runs narrow rounds only
    before = []
    for t in ts:
        _, s_t = call(ops, ei, None, n, t, o_n, seed=7)
        if s_t["n_rounds_narrow"] == s_t["n_rounds"]:
            before.append(t)
    assert before and len(before) < len(ts) and before == ts[:len(before)], f"segment boundaries on both sides of the hand-over: {before} of {ts}"
    sc, ptr = ops.approximate_cholesky_depths(torch.from_numpy(ei).cuda(), None, n, ts, "degree", o_n, seed=7)
    st = dict(ops.last_stats)
    assert st["n_retries"] == 0, st
    assert_kernel(ops, _lib.KERNEL_ROUND, f"depths degree/{o_n}")
    sc, ptr = sc.cpu().numpy(), ptr.numpy()
    for k, t in enumerate(ts):
        ref = oracle.approximate_cholesky(ei, None, n, t, "degree", o_n, shuffle_seed=7)
        assert_same(sc[int(ptr[k]):int(ptr[k + 1])], ref, f"depths degree/{o_n} snapshot {k} (t={t})")
    assert 0 < st["n_rounds_narrow"] < st["n_rounds"], st


def test_debug_jitter_and_poison_on_a_narrow_case(ops):
    """The debug perturbations of the round kernel (waves sleeping behind its barriers; LDS and workspace starting as one byte
    pattern) on a call that runs both kernels: the rows do not change."""
    n = 12000
    ei = ba_graph(n, 10, 6)
    clean, st = call(ops, ei, None, n, n // 2, "asc")
    assert 0 < st["n_rounds_narrow"] < st["n_rounds"], st
    ops.debug_set_jitter(6)
    try:
        for rep in range(2):
            got, sj = call(ops, ei, None, n, n // 2, "asc")
            assert np.array_equal(got, clean) and 0 < sj["n_rounds_narrow"] < sj["n_rounds"], f"jitter rep {rep}" + _where(got, clean)
    finally:
        ops.debug_set_jitter(0)
    for byte in (0xFF, 0x00, 0x3C):
        ops.debug_set_poison(byte)
        try:
            got, sp = call(ops, ei, None, n, n // 2, "asc")
            assert np.array_equal(got, clean) and 0 < sp["n_rounds_narrow"] < sp["n_rounds"], f"poison {byte:#x}" + _where(got, clean)
        finally:
            ops.debug_set_poison(-1)


@pytest.mark.parametrize("o_n", ["asc", "desc", "random"])
def test_override_off_gives_the_same_rows(ops, monkeypatch, o_n):
    """RLAP_NARROW=0 runs the 32-slot kernel alone, RLAP_NARROW=1 (the default) the pair: equal rows."""
    n = 15000
    ei = ba_graph(n, 10, 8)
    monkeypatch.setenv("RLAP_NARROW", "1")
    on, st_on = call(ops, ei, None, n, n // 2, o_n)
    monkeypatch.setenv("RLAP_NARROW", "0")
    off, st_off = call(ops, ei, None, n, n // 2, o_n)
    monkeypatch.delenv("RLAP_NARROW")
    assert st_off["n_rounds_narrow"] == 0 and st_on["n_rounds_narrow"] > 0, (st_on, st_off)
    assert on.shape == off.shape and np.array_equal(on, off), _where(on, off)
