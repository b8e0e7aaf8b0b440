"""CPU check of the 16-slot candidate records of the degree order's first round kernel (k_eliminate_batch_t<OV_DEGREE, *, 16, 1024>):
the host mirror's batch driver instantiated with CandT<16> and 256 candidates per round, bit-exact against the oracle.  Columns
longer than 16 slots go to the mirror's single-vertex path here; on the device the 32-slot kernel takes over at that point."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from util import ba_graph, sym_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


@pytest.fixture(scope="module")
def narrow_mirror():
    src = os.path.join(ROOT, "tests", "csrc", "host_mirror_narrow.cc")
    so = os.path.join(ROOT, "tests", "csrc", "libhost_mirror_narrow.so")
    deps = [src, os.path.join(ROOT, "tests", "csrc", "host_mirror.cc")] + [os.path.join(ROOT, "rlap_amd", "csrc", h) for h in ("rlap_core.h", "rlap_flow.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-msse4.2", "-mavx", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.mirror_approx_chol_batch_narrow.restype = ctypes.c_int
    return lib


def _narrow(lib, ei, w, n, t, o_n, B=256, seed=0):
    E = ei.shape[1]
    row, col = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    w = np.ones(E) if w is None else np.ascontiguousarray(w, dtype=np.float64)
    out = ctypes.POINTER(ctypes.c_double)()
    rows = ctypes.c_int64()
    order = np.full(max(n, 1), -1, dtype=np.int64)
    stats = np.zeros(24, dtype=np.int64)
    rc = lib.mirror_approx_chol_batch_narrow(
        ctypes.c_void_p(row.ctypes.data), ctypes.c_void_p(col.ctypes.data), ctypes.c_void_p(w.ctypes.data),
        ctypes.c_int64(E), ctypes.c_int64(n), ctypes.c_int64(t), oracle.O_V["degree"], oracle.O_N[o_n],
        None, ctypes.c_uint64(seed), ctypes.c_int32(4 * E + 64), ctypes.c_int32(B),
        ctypes.byref(out), ctypes.byref(rows), ctypes.c_void_p(order.ctypes.data), ctypes.c_void_p(stats.ctypes.data))
    assert rc == 0
    m = rows.value
    res = np.ctypeslib.as_array(out, shape=(max(m, 1) * 3,))[: 3 * m].copy().reshape(m, 3)
    lib.mirror_free(out)
    return res, order[:n], stats


def _check(lib, name, ei, n, o_n):
    for t in sorted({1, n // 2, n - 1}):
        for wts in (None, sym_weights(ei, n, 5)):
            a, oa = oracle.approximate_cholesky(ei, wts, n, t, "degree", o_n, shuffle_seed=3, return_order=True)
            b, ob, st = _narrow(lib, ei, wts, n, t, o_n, seed=3)
            assert np.array_equal(oa, ob), (name, t, wts is not None)
            assert a.shape == b.shape and np.array_equal(a, b), (name, t, wts is not None)


@pytest.mark.parametrize("o_n", ["asc", "desc", "random"])
@pytest.mark.parametrize("m", [2, 5, 10])
def test_narrow_records_equal_sequential_order_on_ba(narrow_mirror, o_n, m):
    """BA(n, m), m in {2, 5, 10}: unit and tie-free weights, t in {1, n/2, n-1}."""
    for n, seed in ((600, 1), (3000, 2)):
        _check(narrow_mirror, f"BA({n},{m})", ba_graph(n, m, seed), n, o_n)


@pytest.mark.parametrize("o_n", ["asc", "desc", "random"])
@pytest.mark.parametrize("topo", ["hub", "er", "grid", "cliques"])
def test_narrow_records_equal_sequential_order_on_soak_topologies(narrow_mirror, o_n, topo):
    """The other topologies of tests/tools/soak.py: a hub (long columns), uniform random pairs (isolated and degree-1 vertices),
    a grid, a ring of cliques (multi-edges from the first elimination on)."""
    import soak
    c = {"n": 1200, "m": 5, "seed": 77, "topo": topo}
    ei = soak.make_graph(c, 0)
    _check(narrow_mirror, topo, ei, c["n"], o_n)


def test_narrow_rounds_are_fewer_while_columns_are_short(narrow_mirror, host_mirror):
    """What the shape is for: over the first quarter of BA(n, 10)'s degree order no column is longer than 16 slots, and 256
    narrow candidates per round need fewer rounds than 128 32-slot ones: a round that ends because all 128 candidates were
    committed goes on with twice the capacity (the mirror has no move cap; at n = 1M, t = n/2 it counts 2,793 rounds against 4,635)."""
    n = 20000
    ei = ba_graph(n, 10, 1)
    _, _, st16 = _narrow(narrow_mirror, ei, None, n, n // 4, "asc", B=256, seed=3)
    from test_core_mirror import _mirror_batch
    _, _, st32 = _mirror_batch(host_mirror, ei, None, n, n // 4, "degree", "asc", 128, seed=3, bc=32)
    print("rounds, singles: 16-slot", int(st16[0]), int(st16[1]), "32-slot", int(st32[0]), int(st32[1]))
    assert st16[1] == st32[1], "no column of the first quarter is longer than 16 slots: the same single-vertex fallbacks"
    assert st16[0] < st32[0], (int(st16[0]), int(st32[0]))
