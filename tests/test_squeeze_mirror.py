"""CPU check of the degree order's squeeze pass (rlap_amd/csrc/rlap_squeeze.hip): the host mirror's 16-slot batch driver calls the
squeeze rule of rlap_core.h (squeeze_rank_col, squeeze_entry -- the statements the kernels run) where the device's 16-slot kernel
hands over, and carries on with 16-slot rounds in the second arena (tests/csrc/host_mirror_squeeze.cc).  Bit-exact against the
oracle; after every squeeze the mirror itself checks the twin links, every column's live sequence in traversal order and the
pool's restart, and reports what failed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle
from util import ba_graph, clique, sym_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def squeeze_mirror():
    src = os.path.join(ROOT, "tests", "csrc", "host_mirror_squeeze.cc")
    so = os.path.join(ROOT, "tests", "csrc", "libhost_mirror_squeeze.so")
    deps = [src, os.path.join(ROOT, "tests", "csrc", "host_mirror.cc")] + [os.path.join(ROOT, "rlap_amd", "csrc", h) for h in ("rlap_core.h", "rlap_flow.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-msse4.2", "-mavx", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.mirror_approx_chol_batch_squeeze.restype = ctypes.c_int
    return lib


def squeeze_call(lib, ei, w, n, t, o_n, seed=3, B=256):
    """(rows, pop order, stats) of the mirror with squeezes; stats[20..27]: host_mirror_squeeze.cc."""
    E = ei.shape[1]
    row, col = np.ascontiguousarray(ei[0]), np.ascontiguousarray(ei[1])
    w = np.ones(E) if w is None else np.ascontiguousarray(w, dtype=np.float64)
    out = ctypes.POINTER(ctypes.c_double)()
    rows = ctypes.c_int64()
    order = np.full(max(n, 1), -1, dtype=np.int64)
    stats = np.zeros(32, dtype=np.int64)
    rc = lib.mirror_approx_chol_batch_squeeze(
        ctypes.c_void_p(row.ctypes.data), ctypes.c_void_p(col.ctypes.data), ctypes.c_void_p(w.ctypes.data),
        ctypes.c_int64(E), ctypes.c_int64(n), ctypes.c_int64(t), oracle.O_V["degree"], oracle.O_N[o_n],
        None, ctypes.c_uint64(seed), ctypes.c_int32(4 * E + 64), ctypes.c_int32(B),
        ctypes.byref(out), ctypes.byref(rows), ctypes.c_void_p(order.ctypes.data), ctypes.c_void_p(stats.ctypes.data))
    assert rc == 0
    m = rows.value
    res = np.ctypeslib.as_array(out, shape=(max(m, 1) * 3,))[: 3 * m].copy().reshape(m, 3)
    lib.mirror_free(out)
    return res, order[:n], stats


CASES = {
    "ba3000_half": (lambda: ba_graph(3000, 10, 2), 3000, 1500),
    "ba3000_all": (lambda: ba_graph(3000, 10, 2), 3000, 2999),
    "ba4096": (lambda: ba_graph(4096, 8, 5), 4096, 2048),
    "k40": (lambda: clique(40), 40, 39),
    "ba100_50": (lambda: ba_graph(100, 50, 4), 100, 99),   # multi-edges with equal weights: the order of equal ids matters
}


@pytest.mark.parametrize("o_n", ["asc", "desc", "random"])
@pytest.mark.parametrize("name", list(CASES))
def test_mirror_with_squeezes_equals_the_oracle(squeeze_mirror, name, o_n):
    make, n, t = CASES[name]
    ei = make()
    for wts in (None, sym_weights(ei, n, 5)):
        a, oa = oracle.approximate_cholesky(ei, wts, n, t, "degree", o_n, shuffle_seed=3, return_order=True)
        b, ob, st = squeeze_call(squeeze_mirror, ei, wts, n, t, o_n)
        what = (name, o_n, "tie_free" if wts is not None else "unit")
        print(what, "squeezes", int(st[20]), "with progress", int(st[21]), "at", int(st[26]), int(st[27]), "rounds", int(st[0]), "singles", int(st[1]))
        assert st[22] == 0, f"{what}: {int(st[22])} entries whose twin does not point back (or lies outside its column)"
        assert st[23] == 0, f"{what}: {int(st[23])} columns whose live sequence changed"
        assert st[24] == 0 and st[25] == 0, f"{what}: pool_top != colptr'[N] ({int(st[24])}), entries out of range ({int(st[25])})"
        assert np.array_equal(oa, ob), what
        assert a.shape == b.shape and np.array_equal(a, b), what
        if name != "ba4096":   # (BA(4096,8), t = n/2 stays within 16 slots under some weights: the pass never runs there)
            assert st[20] >= 1, f"{what}: no column at the head of the queue ever had more than 16 slots -- the case squeezes nothing"


def test_squeeze_carries_the_16_slot_rounds_further(squeeze_mirror):
    """What the pass is for: BA(20000,10), t = n/2 -- both squeezes are followed by 16-slot rounds, and the first column of more
    than 16 LIVE entries comes later than the first of more than 16 slots (the seeds tests/test_gpu_squeeze.py uses)."""
    n = 20000
    ei = ba_graph(n, 10, 1)
    for o_n in ("asc", "desc", "random"):
        for wts in (None, sym_weights(ei, n, 5)):
            a = oracle.approximate_cholesky(ei, wts, n, n // 2, "degree", o_n, shuffle_seed=9)
            b, _, st = squeeze_call(squeeze_mirror, ei, wts, n, n // 2, o_n, seed=9)
            print(o_n, "unit" if wts is None else "tie_free", "squeezes at", int(st[26]), int(st[27]), "with progress", int(st[21]))
            assert st[22] == 0 and st[23] == 0 and st[24] == 0 and st[25] == 0, st[20:28]
            assert a.shape == b.shape and np.array_equal(a, b)
            assert st[20] == 2 and st[21] >= 1 and st[27] > st[26] > 0, st[20:28]
