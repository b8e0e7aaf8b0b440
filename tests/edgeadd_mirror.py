"""Loader of the edge-adding host mirror (tests/csrc/edgeadd_mirror.cc around rlap_amd/csrc/rlap_edgeadd.h), shared by
tests/test_edge_add_cpu.py and the tests/test_gpu_edge_add*.py files.  `run` is one whole call on the host."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "csrc", "edgeadd_mirror.cc")
MAIN = os.path.join(ROOT, "tests", "csrc", "edgeadd_main.cc")
STATUS = {2: "an id outside [0, num_nodes)", 3: "a malformed argument", 9: "beyond the limits"}


class Refused(ValueError):
    def __init__(self, status):
        super().__init__(f"edge add mirror: status {status} ({STATUS.get(status, '?')})")
        self.status = status


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libedgeadd_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    lib = ctypes.CDLL(so)
    i64, u64, ci, vp, dbl = ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    lib.edgeadd_u_add.restype = dbl
    lib.edgeadd_u_add.argtypes = [u64, ci, i64, ci]
    lib.edgeadd_draw.restype = i64
    lib.edgeadd_draw.argtypes = [u64, ci, i64, ci, i64]
    lib.edgeadd_id_bits.restype = ctypes.c_uint
    lib.edgeadd_id_bits.argtypes = [i64]
    lib.edgeadd_pair_key.restype = u64
    lib.edgeadd_pair_key.argtypes = [i64, i64, i64]
    lib.edgeadd_one_sort.restype = ci
    lib.edgeadd_one_sort.argtypes = [i64, ci]
    lib.edgeadd_row_tile.restype = ci
    lib.edgeadd_max_views.restype = ci
    lib.edgeadd_run.restype = i64
    lib.edgeadd_run.argtypes = [vp, vp, vp, i64, i64, vp, i64, u64, ci, vp, vp, vp, vp, vp]
    return lib


def counts_of(E, ratio):
    """num_add of every view: the reference's int(num_edges * ratio) on Python floats."""
    return [int(E * float(r)) for r in np.atleast_1d(np.asarray(ratio, dtype=np.float64)).tolist()]


def run(lib, src, dst, n, w=None, ratio=0.5, seed=0, coalesce=True, num_add=None):
    """One call by the mirror: a dict of rows (M, 3), ptr (K+1,), added (sum of num_add, 2), aptr (K+1,), input_distinct and
    input_sorted.  `num_add` (the counts themselves) overrides `ratio`.  Raises Refused for an input the call refuses."""
    src = np.ascontiguousarray(src, dtype=np.int64)
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    E = src.size
    counts = np.ascontiguousarray(counts_of(E, ratio) if num_add is None else np.atleast_1d(num_add), dtype=np.int64)
    K = counts.size
    total_add = int(counts[(counts > 0) & (counts < 2**24)].sum())
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    rows, ptr = np.full((max(K, 1) * E + total_add + 1, 3), np.nan), np.full(K + 1, -7, dtype=np.int64)
    added, aptr, stats = np.full((total_add + 1, 2), -7, dtype=np.int64), np.full(K + 1, -7, dtype=np.int64), np.zeros(2, dtype=np.int64)
    total = lib.edgeadd_run(src.ctypes.data, dst.ctypes.data, None if wv is None else wv.ctypes.data, E, n, counts.ctypes.data, K,
                            int(seed) & (2**64 - 1), 1 if coalesce else 0, rows.ctypes.data, ptr.ctypes.data, added.ctypes.data, aptr.ctypes.data,
                            stats.ctypes.data)
    if total < 0:
        raise Refused(-total)
    return {"rows": rows[:total].copy(), "ptr": ptr, "added": added[:total_add].copy(), "aptr": aptr, "input_distinct": int(stats[0]),
            "input_sorted": int(stats[1])}
