"""Loader of the node-sampling host mirror (tests/csrc/nodesample_mirror.cc around rlap_amd/csrc/rlap_nodesample.h), shared by
tests/test_node_sample_cpu.py and the tests/test_gpu_node_sample*.py files.  `run` is one whole call on the host."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "csrc", "nodesample_mirror.cc")
MAIN = os.path.join(ROOT, "tests", "csrc", "nodesample_main.cc")
SCHEMES = {"drop": 0, "walk": 1}
STATUS = {2: "an id outside [0, num_nodes)", 3: "a malformed argument", 9: "beyond the limits"}


class Refused(ValueError):
    def __init__(self, status):
        super().__init__(f"node sample mirror: status {status} ({STATUS.get(status, '?')})")
        self.status = status


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libnodesample_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    lib = ctypes.CDLL(so)
    i64, u64, ci, vp, dbl = ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    lib.nodesample_u_node.restype = dbl
    lib.nodesample_u_node.argtypes = [u64, ci, i64]
    lib.nodesample_u_walk.restype = dbl
    lib.nodesample_u_walk.argtypes = [u64, ci, i64, i64, i64]
    lib.nodesample_pick.restype = i64
    lib.nodesample_pick.argtypes = [dbl, i64]
    lib.nodesample_row_tile.restype = ci
    lib.nodesample_max_views.restype = ci
    lib.nodesample_max_walk_length.restype = i64
    lib.nodesample_run.restype = i64
    lib.nodesample_run.argtypes = [vp, vp, vp, i64, i64, ci, vp, vp, i64, i64, u64, vp, vp, vp, vp]
    return lib


def run(lib, src, dst, n, w=None, scheme="drop", p=0.5, num_seeds=None, walk_length=10, seed=0):
    """One call by the mirror: a dict of rows (M, 3), ptr (K+1,), nodes (K, N) bool and, for "walk", walks (sum of num_seeds,
    walk_length + 1).  Raises Refused for an input the call refuses."""
    src = np.ascontiguousarray(src, dtype=np.int64)
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    walk = scheme == "walk"
    ps = np.ascontiguousarray(np.atleast_1d(np.asarray(p, dtype=np.float64)))
    ns = np.ascontiguousarray(np.atleast_1d(np.asarray(num_seeds if walk else 0, dtype=np.int64)))
    E, K = src.size, (ns.size if walk else ps.size)
    wv = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    rows, ptr = np.full((max(K * E, 1), 3), np.nan), np.full(K + 1, -7, dtype=np.int64)
    nodes = np.full((K, max(n, 1)), 7, dtype=np.uint8)
    walkers = int(ns.sum()) if walk and ((ns >= 0) & (ns < 2**31)).all() and ns.size <= 32 else 0   # (a call that is refused writes no walk)
    walks = np.full((walkers, max(int(walk_length), 0) + 1 if int(walk_length) <= 1024 else 1), -7, dtype=np.int64)
    total = lib.nodesample_run(src.ctypes.data, dst.ctypes.data, None if wv is None else wv.ctypes.data, E, n, SCHEMES.get(scheme, scheme),
                               None if walk else ps.ctypes.data, ns.ctypes.data if walk else None, K, int(walk_length), int(seed) & (2**64 - 1),
                               rows.ctypes.data, ptr.ctypes.data, nodes.ctypes.data, walks.ctypes.data if walk else None)
    if total < 0:
        raise Refused(-total)
    out = {"rows": rows[:total].copy(), "ptr": ptr, "nodes": nodes[:, :n].astype(bool)}
    if walk:
        out["walks"] = walks
    return out
