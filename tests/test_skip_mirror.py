"""CPU check of the round kernels' skip rule (rlap_core.h::cand_touches): the degree order's rounds on the host
(tests/csrc/host_mirror_skip.cc), 16-slot records up to the hand-over and 32-slot records behind it, or 32-slot records alone, where
the target counts, the contended list, the replay and the commit see only the (candidate, target) pairs the predicate passes.
Bit-exact against the oracle, rows and pop order.  The drivers have no move cap and no record cap; what they count beside the
result -- touched pairs over all pairs, contended records with and without the rule -- is printed, and the two counts are checked
for what the rule promises: it only ever removes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
from util import ba_graph, clique, sym_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_skip_mirror():
    src = os.path.join(ROOT, "tests", "csrc", "host_mirror_skip.cc")
    so = os.path.join(ROOT, "tests", "csrc", "libhost_mirror_skip.so")
    deps = [src, os.path.join(ROOT, "tests", "csrc", "host_mirror.cc")] + [os.path.join(ROOT, "rlap_amd", "csrc", h) for h in ("rlap_core.h", "rlap_flow.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-msse4.2", "-mavx", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.mirror_approx_chol_batch_skip.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def skip_mirror():
    return load_skip_mirror()


STATS = ("rounds", "singles", "rounds_narrow", "pairs", "pairs_touched", "contended_all", "contended_touched", "complex", "complex_all", "handover_at")


def skip_call(lib, ei, w, n, t, o_n, bc, seed=3, B=192, B32=128):
    """(rows, pop order, stats by name) of the mirror with the rule; bc = 16: both record sizes, 32: the 32-slot rounds alone."""
    E = ei.shape[1]
    row, col = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    w = np.ones(E) if w is None else np.ascontiguousarray(w, dtype=np.float64)
    out = ctypes.POINTER(ctypes.c_double)()
    rows = ctypes.c_int64()
    order = np.full(max(n, 1), -1, dtype=np.int64)
    stats = np.zeros(16, dtype=np.int64)
    rc = lib.mirror_approx_chol_batch_skip(
        ctypes.c_void_p(row.ctypes.data), ctypes.c_void_p(col.ctypes.data), ctypes.c_void_p(w.ctypes.data),
        ctypes.c_int64(E), ctypes.c_int64(n), ctypes.c_int64(t), oracle.O_V["degree"], oracle.O_N[o_n],
        None, ctypes.c_uint64(seed), ctypes.c_int32(4 * E + 64), ctypes.c_int(bc), ctypes.c_int32(B), ctypes.c_int32(B32),
        ctypes.byref(out), ctypes.byref(rows), ctypes.c_void_p(order.ctypes.data), ctypes.c_void_p(stats.ctypes.data))
    assert rc == 0
    m = rows.value
    res = np.ctypeslib.as_array(out, shape=(max(m, 1) * 3,))[: 3 * m].copy().reshape(m, 3)
    lib.mirror_free(out)
    return res, order[:n], dict(zip(STATS, (int(s) for s in stats)))


CASES = {
    "ba300_all": (lambda: ba_graph(300, 10, 2), 300, 299),
    "ba3000_half": (lambda: ba_graph(3000, 10, 2), 3000, 1500),
    "ba3000_all": (lambda: ba_graph(3000, 10, 2), 3000, 2999),
    "ba4096": (lambda: ba_graph(4096, 8, 5), 4096, 2048),
    "k40": (lambda: clique(40), 40, 39),          # keys beyond n: every neighbour's key passes n on the way
    "ba100_50": (lambda: ba_graph(100, 50, 4), 100, 99),   # multi-edges with equal weights, keys beyond n
}

_ref = {}


def reference(name, o_n, weights):
    """The oracle's rows and pop order of a case, computed once for both record sizes."""
    key = (name, o_n, weights)
    if key not in _ref:
        make, n, t = CASES[name]
        ei = make()
        wts = None if weights == "unit" else sym_weights(ei, n, 5)
        _ref[key] = (ei, wts) + tuple(oracle.approximate_cholesky(ei, wts, n, t, "degree", o_n, shuffle_seed=3, return_order=True))
    return _ref[key]


@pytest.mark.parametrize("bc", [16, 32])
@pytest.mark.parametrize("weights", ["unit", "tie_free"])
@pytest.mark.parametrize("o_n", ["asc", "desc", "random"])
@pytest.mark.parametrize("name", list(CASES))
def test_mirror_with_the_skip_rule_equals_the_oracle(skip_mirror, name, o_n, weights, bc):
    _, n, t = CASES[name]
    ei, wts, a, oa = reference(name, o_n, weights)
    b, ob, st = skip_call(skip_mirror, ei, wts, n, t, o_n, bc)
    what = (name, o_n, weights, bc)
    print(what, st)
    assert np.array_equal(oa, ob), what
    assert a.shape == b.shape and np.array_equal(a, b), what
    # the rule only removes: pairs, contended records, and candidates the keys-beyond-n test sends to the single-vertex path
    assert st["pairs_touched"] <= st["pairs"], st
    if name != "k40":   # (every vertex of the clique meets multi-edges or more than 32 entries: it goes by the single-vertex path alone)
        assert st["pairs_touched"] > 0, st
    assert st["contended_touched"] <= st["contended_all"], st
    assert st["complex"] <= st["complex_all"], st
    assert st["rounds"] > 0 and (bc == 16 or st["rounds_narrow"] == 0), st
    if name.startswith("ba3000") and bc == 16:
        assert 0 < st["rounds_narrow"] < st["rounds"] and st["handover_at"] > 0, st   # both record sizes and the hand-over


def test_the_rule_removes_about_half_the_pairs_on_unit_weights(skip_mirror):
    """Unit weights: position j of m goes unpicked with probability (m-1-j)/(m-1), so about half of a candidate's pairs are untouched
    while the columns still hold what the generator gave them -- the share the rule is built on (BA(3000,10), first half)."""
    ei, wts, _, _ = reference("ba3000_half", "asc", "unit")
    _, _, st = skip_call(skip_mirror, ei, wts, 3000, 1500, "asc", 16)
    share = st["pairs_touched"] / st["pairs"]
    print(f"touched {st['pairs_touched']} of {st['pairs']} pairs ({share:.3f}); contended records {st['contended_touched']} with the rule, {st['contended_all']} without")
    assert 0.35 < share < 0.65, st
    assert st["contended_touched"] < st["contended_all"], st
