"""The output pass's capacity tiers (rlap_output.hip): k_sc_tierlists sends a surviving column to one of eight kernels by its extent
(slots in use, dead entries included), with the edges 32, 64, 192, 512, 1024, 2048, 7168 and 65535.  Every call here is compared bit
for bit with the oracle.

Stars with num_remove = 0: nothing is eliminated, so the hub's extent is exactly n - 1 and each edge is met from both sides; 65,536
is the one-lane serial form in global scratch.

Wheels (hub 0 joined to every vertex of a ring of n - 1) with num_remove = t = n // 4 in degree order: a ring vertex has three
neighbours, the hub and one on either side, and keeps at most three (eliminating a vertex only joins its neighbours to each other: the
next ring vertex takes its place); eliminating a vertex of m neighbours samples m - 1 new edges, so at most two entries are appended
to the hub's column per elimination.  The hub's
extent therefore lies in [n - 1, n - 1 + 2 t], and for the sizes below that whole range sits inside one tier, so that each tier's
kernel walks appended chunks, not only a CSR segment:

    n       [n - 1, n - 1 + 2 (n // 4)]   tier
    40      [39, 59]                      (32, 64]
    100     [99, 149]                     (64, 192]
    300     [299, 449]                    (192, 512]
    600     [599, 899]                    (512, 1024]
    1200    [1199, 1799]                  (1024, 2048]
    4000    [3999, 5999]                  (2048, 7168]
    20000   [19999, 29999]                (7168, 65535]
    70000   [69999, 104999]               beyond 65535

(the ring vertices' own columns go through the tier of at most 32 slots).  n_retries is not asserted: the calls of 65,536 and 70,000
vertices may grow the scratch once."""
import numpy as np
import pytest
import torch

import oracle
from test_gpu_parity import assert_same, gpu_call
from util import star, sym_weights, symmetrize

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::rlap_amd.ops.DataflowFallbackWarning")]

STAR_EXTENTS = (32, 33, 64, 65, 192, 193, 512, 513, 1024, 1025, 2048, 2049, 7168, 7169, 65535, 65536)
WHEEL_SIZES = (40, 100, 300, 600, 1200, 4000, 20000, 70000)
ORDERS = ("asc", "desc", "random")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def wheel(n):
    """Hub 0 joined to the ring 1, 2, .., n - 1, 1."""
    ring = np.arange(1, n, dtype=np.int64)
    a = np.concatenate([np.zeros(n - 1, dtype=np.int64), ring])
    b = np.concatenate([ring, np.roll(ring, -1)])
    return symmetrize(a, b, n)


def weightings(ei, n):
    return (("unit", None), ("weighted", sym_weights(ei, n, 2)))   # all ties | tie-free


@pytest.mark.parametrize("o_n", ORDERS)
def test_star_hub_on_both_sides_of_every_tier_edge(ops, o_n):
    for ext in STAR_EXTENTS:
        n = ext + 1
        ei = star(n)
        for name, w in weightings(ei, n):
            a = oracle.approximate_cholesky(ei, w, n, 0, "degree", o_n, shuffle_seed=8)
            b = gpu_call(ops, ei, w, n, 0, "degree", o_n, seed=8)
            assert_same(b, a, f"star, hub extent {ext}, {o_n}, {name}")


@pytest.mark.parametrize("o_n", ORDERS)
def test_wheel_hub_with_appended_chunks_in_every_tier(ops, o_n):
    for n in WHEEL_SIZES:
        ei = wheel(n)
        for name, w in weightings(ei, n):
            a = oracle.approximate_cholesky(ei, w, n, n // 4, "degree", o_n, shuffle_seed=8)
            b = gpu_call(ops, ei, w, n, n // 4, "degree", o_n, seed=8)
            assert_same(b, a, f"wheel{n} t={n // 4}, {o_n}, {name}")


def test_batched_wheels_keyed_order_in_two_tiers(ops):
    """One batched call of the 300- and 1200-vertex wheels, o_n = random: the key base is per graph (graph g orders with seed + g)."""
    from rlap_amd import graphs
    ns = [300, 1200]
    eis = [wheel(n) for n in ns]
    ws = [sym_weights(ei, n, 2) for ei, n in zip(eis, ns)]
    big, node_ptr = graphs.batch_disjoint([torch.from_numpy(ei) for ei in eis], ns)
    sc, rp = ops.approximate_cholesky_batched(big.cuda(), torch.from_numpy(np.concatenate(ws)).cuda(), node_ptr, [n // 4 for n in ns],
                                              "degree", "random", seed=8)
    sc = sc.cpu().numpy()
    for g, n in enumerate(ns):
        ref = oracle.approximate_cholesky(eis[g], ws[g], n, n // 4, "degree", "random", shuffle_seed=8 + g)
        got = sc[int(rp[g]):int(rp[g + 1])].copy()
        got[:, :2] -= int(node_ptr[g])
        assert_same(got, ref, f"batched wheel{n}")
