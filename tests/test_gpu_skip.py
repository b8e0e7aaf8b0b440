"""The round kernels' skip rule (rlap_core.h::cand_touches): the replay phase of k_eliminate_batch_t sees only the (candidate,
target) pairs an elimination touches -- a pick names the target, or it is the candidate's last neighbour (degree order); it is the
chosen neighbour (coarsening).  The others keep their key and get nothing appended: no key load, no place in the round's table of
shared targets, no contended record.  Every case is bit-exact against the CPU oracle on the round kernel with n_retries == 0;
tests/test_skip_mirror.py checks the same rule on the CPU."""
import numpy as np
import pytest
import torch

import oracle
from rlap_amd import _lib
from util import assert_kernel, ba_graph, clique, sym_weights, symmetrize
from test_gpu_parity import assert_same, gpu_call, _where
from test_gpu_narrow import call

pytestmark = [pytest.mark.gpu]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def wheel(n):
    """Hub 0 joined to every vertex of the ring 1 .. n-1."""
    ring = np.arange(1, n, dtype=np.int64)
    nxt = np.where(ring + 1 < n, ring + 1, 1)
    return symmetrize(np.concatenate([np.zeros(n - 1, dtype=np.int64), ring]), np.concatenate([ring, nxt]), n)


def two_hubs(leaves):
    """Hubs 0 and 1 with `leaves` leaves each; all the leaves form one ring."""
    n = 2 + 2 * leaves
    leaf = np.arange(2, n, dtype=np.int64)
    hub = (leaf - 2) // leaves
    nxt = np.where(leaf + 1 < n, leaf + 1, 2)
    return symmetrize(np.concatenate([hub, leaf]), np.concatenate([leaf, nxt]), n), n


@pytest.mark.parametrize("weights", ["unit", "tie_free"])
@pytest.mark.parametrize("o_n", ["asc", "desc", "random"])
def test_small_graph_to_its_last_vertices(ops, o_n, weights):
    """BA(300,10), t = n - 1: rounds of few candidates, and the last vertices, where the Dec of the last neighbour is not allowed."""
    n = 300
    ei = ba_graph(n, 10, 2)
    _, st = call(ops, ei, None if weights == "unit" else sym_weights(ei, n, 5), n, n - 1, o_n, seed=3)
    assert st["n_rounds"] > 0, st


@pytest.mark.parametrize("weights", ["unit", "tie_free"])
@pytest.mark.parametrize("t", [1500, 2999])
def test_both_shapes_and_the_hand_over(ops, t, weights):
    """BA(3000,10): the 16-slot kernel up to pop 943 or so, the 32-slot kernel behind it.
    t = n - 1: eliminated to its last vertex the graph appends more entries and draws more uniforms than a handle's first guess
    allows (pool: nnz + 16 n slots, uniforms: nnz + 1024), so a handle that has not grown yet repeats the call with larger tables.
    Measured on a fresh handle, this build and the one before it alike: n_retries 2, retry_causes 0b1010 (pool, uniforms).  That
    growth is the library's, not the round kernel's: the case lets it happen in a first call, which may repeat itself for those
    two reasons only and must return the oracle's rows, and then makes the checks of every case here on a second one."""
    n = 3000
    ei = ba_graph(n, 10, 2)
    w = None if weights == "unit" else sym_weights(ei, n, 5)
    if t == n - 1:
        first = gpu_call(ops, ei, w, n, t, "degree", "asc", seed=3, kernel=_lib.KERNEL_ROUND)
        causes = ops.last_stats["retry_causes"]
        assert causes & ~(_lib.RETRY_POOL | _lib.RETRY_RNG) == 0, f"retry_causes {causes:#b}"
        assert_same(first, oracle.approximate_cholesky(ei, w, n, t, "degree", "asc", shuffle_seed=3), f"t={t}, first call")
    _, st = call(ops, ei, w, n, t, "asc", seed=3)
    assert 0 < st["n_rounds_narrow"] < st["n_rounds"], st


def test_hub_adjacent_to_every_candidate(ops):
    """A wheel: the hub is a target of every candidate of every round and picked by few of them.  (Eliminating a ring vertex joins
    its ring neighbour to the hub a second time, so after the first rounds most vertices meet a multi-edge and go by the
    single-vertex path: tests/test_skip_mirror.py's driver counts 997 of them in 999 rounds.)"""
    n = 2000
    _, st = call(ops, wheel(n), None, n, n // 2, "asc", seed=3)
    assert st["n_rounds"] > 0, st


def test_two_hubs_shared_by_their_leaves(ops):
    """Two hubs, 1,000 leaves each, leaves in a ring: a hub is the last neighbour (j == m-1) of many candidates of a round at once.
    (As with the wheel, multi-edges with the hubs soon send most vertices to the single-vertex path.)"""
    ei, n = two_hubs(1000)
    _, st = call(ops, ei, None, n, n // 2, "asc", seed=3)
    assert st["n_rounds"] > 0, st


@pytest.mark.parametrize("name", ["ba100_50", "k40"])
def test_multi_edges_and_keys_beyond_n(ops, name):
    """Dense graphs: multi-edges send candidates to the single-vertex path, and keys pass n -- the rule may send fewer candidates
    there than the key test alone did, the rows stay the oracle's."""
    if name == "k40":
        n = 40; ei = clique(n)
    else:
        n = 100; ei = ba_graph(n, 50, 4)
    _, st = call(ops, ei, None, n, n - 1, "asc", seed=3)
    assert st["n_rounds"] + st["n_singles"] > 0, st


def test_coarsening_order_shares_the_loop(ops):
    """BA(3000,7), coarsen/asc: only the chosen neighbour of a candidate is touched."""
    n = 3000
    ei = ba_graph(n, 7, 2)
    got = ops.approximate_cholesky(torch.from_numpy(ei).cuda(), None, n, n // 2, "coarsen", "asc", seed=3).numpy()
    st = dict(ops.last_stats)
    assert_kernel(ops, _lib.KERNEL_ROUND, "coarsen/asc")
    assert st["n_retries"] == 0 and st["n_rounds"] > 0, st
    assert_same(got, oracle.approximate_cholesky(ei, None, n, n // 2, "coarsen", "asc", shuffle_seed=3), "BA(3000,7) coarsen/asc")


def test_64_slot_shape_keeps_every_pair(ops, monkeypatch):
    """4 x BA(4096,8) in one call, o_v = random on the round kernel (64-slot candidates): the path without the rule, same loop."""
    from rlap_amd import graphs
    monkeypatch.setenv("RLAP_FLOW", "0")
    n, G = 4096, 4
    eis = [ba_graph(n, 8, 5 + g) for g in range(G)]
    big, node_ptr = graphs.batch_disjoint([torch.from_numpy(e) for e in eis], [n] * G)
    perms = [np.random.RandomState(g).permutation(n) for g in range(G)]
    sc, row_ptr = ops.approximate_cholesky_batched(big.cuda(), None, node_ptr, [n // 2] * G, "random", "asc",
                                                   perm=torch.from_numpy(np.concatenate(perms)), seed=5)
    st = dict(ops.last_stats)
    assert_kernel(ops, _lib.KERNEL_ROUND, "4 x BA(4096,8) random/asc")
    assert st["n_retries"] == 0 and st["n_rounds"] > 0, st
    sc = sc.cpu().numpy()
    for g in range(G):
        ref = oracle.approximate_cholesky(eis[g], None, n, n // 2, "random", "asc", perm=perms[g], shuffle_seed=5 + g)
        b = sc[int(row_ptr[g]):int(row_ptr[g + 1])].copy()
        b[:, :2] -= int(node_ptr[g])
        assert_same(b, ref, f"graph {g} random/asc")


def test_debug_jitter_and_poison(ops):
    """The debug perturbations of the round kernel on a call that runs both shapes: waves sleeping behind the barriers (a record
    parked in front of a barrier and read behind it), then LDS starting as one byte pattern (a record that was never written)."""
    n = 3000
    ei = ba_graph(n, 10, 2)
    clean, st = call(ops, ei, None, n, n // 2, "asc", seed=3)
    assert 0 < st["n_rounds_narrow"] < st["n_rounds"], st
    ops.debug_set_jitter(6)
    try:
        got, sj = call(ops, ei, None, n, n // 2, "asc", seed=3)
        assert np.array_equal(got, clean) and 0 < sj["n_rounds_narrow"] < sj["n_rounds"], "jitter" + _where(got, clean)
    finally:
        ops.debug_set_jitter(0)
    ops.debug_set_poison(0xFF)
    try:
        got, sp = call(ops, ei, None, n, n // 2, "asc", seed=3)
        assert np.array_equal(got, clean) and 0 < sp["n_rounds_narrow"] < sp["n_rounds"], "poison 0xff" + _where(got, clean)
    finally:
        ops.debug_set_poison(-1)
