"""Loader of the edge-dropping host mirror (tests/csrc/edgedrop_mirror.cc around rlap_amd/csrc/rlap_edgedrop.h), shared by
tests/test_edge_drop_cpu.py and the tests/test_gpu_edge_drop*.py files.  `run` is one whole call on the host."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "csrc", "edgedrop_mirror.cc")
MAIN = os.path.join(ROOT, "tests", "csrc", "edgedrop_main.cc")
SCHEMES = {"uniform": 0, "degree": 1, "pagerank": 2, "eigenvector": 3}
STATUS = {2: "an id outside [0, num_nodes)", 3: "a malformed argument", 9: "beyond the limits"}


class Refused(ValueError):
    def __init__(self, status):
        super().__init__(f"edge drop mirror: status {status} ({STATUS.get(status, '?')})")
        self.status = status


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libedgedrop_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    lib = ctypes.CDLL(so)
    i64, u64, ci, vp, dbl = ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    lib.edgedrop_coin.restype = dbl
    lib.edgedrop_coin.argtypes = [u64, ci, i64]
    for name in ("edgedrop_tile", "edgedrop_row_tile", "edgedrop_max_views"):
        getattr(lib, name).restype = ci
    lib.edgedrop_pair_key_bits.restype = ctypes.c_uint
    lib.edgedrop_pair_key_bits.argtypes = [i64]
    lib.edgedrop_run.restype = i64
    lib.edgedrop_run.argtypes = [vp, vp, vp, i64, i64, ci, ci, vp, i64, dbl, u64, dbl, i64, dbl, i64] + [vp] * 9
    return lib


def run(lib, src, dst, n, w=None, p=0.5, scheme="uniform", threshold=0.7, seed=0, aggr="sink", pr_damp=0.85, pr_iters=10, evc_tol=1e-6,
        evc_max_iter=1000):
    """One call by the mirror: a dict of rows (M, 3), ptr (K+1,), mask (K, E) bool, q and u (K, E), centrality, node_weight (N,),
    iters, converged.  Raises Refused for an input the call refuses."""
    src = np.ascontiguousarray(src, dtype=np.int64)
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    ps = np.ascontiguousarray(np.atleast_1d(np.asarray(p, dtype=np.float64)))
    E, K = src.size, ps.size
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    rows, ptr = np.full((max(K * E, 1), 3), np.nan), np.full(K + 1, -7, dtype=np.int64)
    mask, q, u = np.zeros((K, E), dtype=np.uint8), np.full((K, E), np.nan), np.full((K, E), np.nan)
    cen, nw = np.full(max(n, 1), np.nan), np.full(max(n, 1), np.nan)
    iters, conv = ctypes.c_int32(-1), ctypes.c_int32(-1)
    total = lib.edgedrop_run(src.ctypes.data, dst.ctypes.data, None if wv is None else wv.ctypes.data, E, n, SCHEMES[scheme],
                             {"sink": 0, "source": 1}[aggr], ps.ctypes.data, K, float(threshold), int(seed) & (2**64 - 1), float(pr_damp),
                             int(pr_iters), float(evc_tol), int(evc_max_iter), rows.ctypes.data, ptr.ctypes.data, mask.ctypes.data,
                             q.ctypes.data, u.ctypes.data, cen.ctypes.data, nw.ctypes.data, ctypes.byref(iters), ctypes.byref(conv))
    if total < 0:
        raise Refused(-total)
    return {"rows": rows[:total].copy(), "ptr": ptr, "mask": mask.astype(bool), "q": q, "u": u, "centrality": cen[:n].copy(),
            "node_weight": nw[:n].copy(), "iters": int(iters.value), "converged": bool(conv.value)}
