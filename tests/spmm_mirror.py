"""Loader of the propagation's host mirror (tests/csrc/spmm_mirror.cc around rlap_amd/csrc/rlap_spmm.h), shared by
tests/test_propagate_cpu.py and tests/test_gpu_propagate.py."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_spmm.h")
SRC = os.path.join(ROOT, "tests", "csrc", "spmm_mirror.cc")


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libspmm_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    lib.spmm_chunk.restype = ci
    lib.spmm_chunk.argtypes = []
    lib.spmm_list.restype = dbl
    lib.spmm_list.argtypes = [i64, vp, vp, ci, dbl, dbl]
    lib.spmm_entries.restype = None
    lib.spmm_entries.argtypes = [i64, vp, vp, vp, i64, i64, vp, ci, ci, vp]
    lib.readout_dispatch.restype = None
    lib.readout_dispatch.argtypes = [i64, ci, ci, vp]
    return lib


def readout_dispatch(lib, F, elem_bytes, aligned16):
    """{"vec", "lanes", "lg", "ftiles"} of rlap_readout.h's dispatch rule: which kernel a readout of F columns takes."""
    out = np.zeros(4, dtype=np.int64)
    lib.readout_dispatch(int(F), int(elem_bytes), 1 if aligned16 else 0, out.ctypes.data)
    return {"vec": bool(out[0]), "lanes": int(out[1]), "lg": int(out[2]), "ftiles": int(out[3])}


def list_sum(lib, c, x, loop=None):
    """One element by the mirror: the terms c[e] * x[e] in order, then the loop term (c_loop, x_loop) if given."""
    c = np.ascontiguousarray(c, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert c.shape == x.shape and c.ndim == 1
    cl, xl = loop if loop is not None else (0.0, 0.0)
    return np.float64(lib.spmm_list(c.size, c.ctypes.data, x.ctypes.data, 1 if loop is not None else 0, float(cl), float(xl)))


def entries(lib, src, dst, val, num_nodes, x, loops, transpose):
    """y (num_nodes, F) of one entry list by the mirror; all arrays numpy, x float64 (num_nodes, F)."""
    src = np.ascontiguousarray(src, dtype=np.int64)
    dst = np.ascontiguousarray(dst, dtype=np.int64)
    val = np.ascontiguousarray(val, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.shape[0] == num_nodes and src.shape == dst.shape == val.shape
    y = np.empty_like(x)
    lib.spmm_entries(src.size, src.ctypes.data, dst.ctypes.data, val.ctypes.data, num_nodes, x.shape[1], x.ctypes.data,
                     1 if loops else 0, 1 if transpose else 0, y.ctypes.data)
    return y
