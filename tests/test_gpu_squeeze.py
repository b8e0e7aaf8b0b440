"""The degree order's squeeze passes (rlap_amd/csrc/rlap_squeeze.hip): between launches of the 16-slot round kernel every surviving
column is rewritten into a second arena without its dead entries.  The size gate keeps the pass to large graphs; RLAP_SQUEEZE=1
switches it on for the small ones here.  Every case is bit-exact against the CPU oracle on the round kernel with n_retries == 0
(tests/test_gpu_narrow.py::call); rlap_stats.n_squeezes counts the passes behind which the 16-slot kernel committed another round.
That the graphs below hand over with at most 16 live entries at the head of the queue is checked on the CPU by
tests/test_squeeze_mirror.py::test_squeeze_carries_the_16_slot_rounds_further (same generator, same seeds)."""
import numpy as np
import pytest
import torch

import oracle
from rlap_amd import _lib
from util import assert_kernel, ba_graph, path, sym_weights
from test_gpu_parity import assert_same, _where
from test_gpu_narrow import call

pytestmark = [pytest.mark.gpu]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture
def squeeze_on(monkeypatch):
    monkeypatch.setenv("RLAP_SQUEEZE", "1")
    return monkeypatch


@pytest.mark.parametrize("o_n", ["asc", "desc", "random"])
@pytest.mark.parametrize("weights", ["unit", "tie_free"])
def test_squeezes_carry_the_16_slot_kernel_further(ops, squeeze_on, o_n, weights):
    """BA(20000,10), t = n/2: the hand-overs fall near pops 6,200 and 7,600 of 10,000 with no more than 16 live entries at the head
    of the queue, so both passes are followed by 16-slot rounds."""
    n = 20000
    ei = ba_graph(n, 10, 1)
    w = None if weights == "unit" else sym_weights(ei, n, 5)
    on, st_on = call(ops, ei, w, n, n // 2, o_n)
    squeeze_on.setenv("RLAP_SQUEEZE", "0")
    off, st_off = call(ops, ei, w, n, n // 2, o_n)
    print(f"n_squeezes {st_on['n_squeezes']}; n_rounds_narrow {st_on['n_rounds_narrow']} (pass off: {st_off['n_rounds_narrow']}); n_rounds {st_on['n_rounds']} ({st_off['n_rounds']})")
    assert st_off["n_squeezes"] == 0, st_off
    assert st_on["n_squeezes"] >= 1, st_on
    assert st_on["n_rounds_narrow"] > st_off["n_rounds_narrow"], (st_on, st_off)
    assert on.shape == off.shape and np.array_equal(on, off), _where(on, off)


@pytest.mark.parametrize("o_n", ["asc", "random"])
def test_32_slot_kernel_and_single_vertex_path_on_a_squeezed_arena(ops, squeeze_on, o_n):
    """BA(3000,10), t = n - 1: behind the last hand-over the 32-slot kernel and its single-vertex path run in the arena the second
    pass wrote, with hub columns (a wave each in the pass) long before and after."""
    n = 3000
    _, st = call(ops, ba_graph(n, 10, 2), None, n, n - 1, o_n)
    assert st["n_squeezes"] >= 1 and 0 < st["n_rounds_narrow"] < st["n_rounds"] and st["n_singles"] > 0, st


def test_first_candidate_already_wide(ops, squeeze_on):
    """BA(3000,20): the lowest degree is 20 -- two passes without progress, and the rows of a call with the pass off."""
    n = 3000
    ei = ba_graph(n, 20, 2)
    on, st = call(ops, ei, None, n, n // 2, "asc")
    assert st["n_squeezes"] == 0 and st["n_rounds_narrow"] == 0 and st["n_rounds"] > 0, st
    squeeze_on.setenv("RLAP_SQUEEZE", "0")
    off, st_off = call(ops, ei, None, n, n // 2, "asc")
    assert st_off["n_squeezes"] == 0 and on.shape == off.shape and np.array_equal(on, off), _where(on, off)


def test_graph_that_never_hands_over(ops, squeeze_on):
    """path(5000), t = n - 1: the 16-slot kernel finishes the elimination, the passes run over what is left, and the output pass
    reads the arena the last one wrote."""
    n = 5000
    _, st = call(ops, path(n), None, n, n - 1, "asc")
    assert st["n_squeezes"] == 0 and st["n_rounds"] > 0 and st["n_rounds_narrow"] == st["n_rounds"], st


def test_batch_of_graphs_that_hand_over_at_different_points(ops, squeeze_on):
    """The five graphs of tests/test_gpu_narrow.py's batch in one call: one pass serves all of them, each at its own point of its
    own order; graph g equals a call of its own with seed + g."""
    from rlap_amd import graphs
    spec = [(6000, 3), (5000, 10), (3000, 20), (9000, 8), (4000, 12)]
    eis = [ba_graph(n, m, 50 + g) for g, (n, m) in enumerate(spec)]
    ns = [n for n, _ in spec]
    ts = [n // 2 for n in ns]
    big, node_ptr = graphs.batch_disjoint([torch.from_numpy(e) for e in eis], ns)
    sc, row_ptr = ops.approximate_cholesky_batched(big.cuda(), None, node_ptr, ts, "degree", "asc", seed=5)
    st = dict(ops.last_stats)
    assert_kernel(ops, _lib.KERNEL_ROUND, "batch degree/asc")
    assert st["n_retries"] == 0, st
    sc = sc.cpu().numpy()
    each = []
    for g, (n, m) in enumerate(spec):
        ref = oracle.approximate_cholesky(eis[g], None, n, ts[g], "degree", "asc", shuffle_seed=5 + g)
        b = sc[int(row_ptr[g]):int(row_ptr[g + 1])].copy()
        b[:, :2] -= int(node_ptr[g])
        assert_same(b, ref, f"graph {g} BA({n},{m})")
        own, sg = call(ops, eis[g], None, n, ts[g], "asc", seed=5 + g)
        assert np.array_equal(own, b), f"graph {g}: the batch and a call of its own differ" + _where(own, b)
        each.append((sg["n_squeezes"], sg["n_rounds_narrow"]))
    assert sum(s for s, _ in each) == st["n_squeezes"] and sum(r for _, r in each) == st["n_rounds_narrow"], (each, st)
    assert st["n_squeezes"] >= 1 and each[2] == (0, 0), (each, st)


def test_rejected_input_fails_as_with_the_pass_off(ops, squeeze_on):
    """An asymmetric input and an out-of-range id: the passes copy nothing, the call fails with the error it fails with when the
    pass is off, and the handle works afterwards."""
    n = 3000
    ei = ba_graph(n, 10, 2)
    w = np.ones(ei.shape[1]); w[7] = 2.0                       # one direction of one edge: not symmetric
    rng = ei.copy(); rng[0, 11] = n + 5                        # an id beyond num_nodes
    errs = {}
    for mode in ("1", "0"):
        squeeze_on.setenv("RLAP_SQUEEZE", mode)
        for name, (e, ww) in {"asymmetric": (ei, w), "range": (rng, None)}.items():
            with pytest.raises(ValueError) as ex:
                ops.approximate_cholesky(torch.from_numpy(e).cuda(), None if ww is None else torch.from_numpy(ww).cuda(), n, n // 2, "degree", "asc")
            errs[(mode, name)] = str(ex.value)
    assert errs[("1", "asymmetric")] == errs[("0", "asymmetric")] and errs[("1", "range")] == errs[("0", "range")], errs
    squeeze_on.setenv("RLAP_SQUEEZE", "1")
    call(ops, ei, None, n, n // 2, "asc")


def test_num_remove_limits(ops, squeeze_on):
    n = 2000
    ei = ba_graph(n, 10, 3)
    for t in (0, 1):
        _, st = call(ops, ei, None, n, t, "asc")
        assert st["n_squeezes"] == 0 and st["n_rounds"] == t and st["n_rounds_narrow"] == t, st
