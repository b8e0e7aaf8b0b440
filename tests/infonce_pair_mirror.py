"""Loader of the symmetric InfoNCE pair's host mirror (tests/csrc/infonce_pair_mirror.cc around rlap_amd/csrc/rlap_infonce.h) and the
float64 restatement 0.5 * (l(a, b) + l(b, a)) built from infonce_mirror.restatement, shared by tests/test_infonce_pair_cpu.py and the
GPU tests; the vectorised exact-data generator of the regime tests (tests/test_gpu_infonce_pair_regimes.py)."""
import ctypes
import os
import subprocess

import numpy as np

import infonce_mirror as im

ROOT = im.ROOT
SRC = os.path.join(ROOT, "tests", "csrc", "infonce_pair_mirror.cc")
THREADS = 8


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libinfonce_pair_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I", os.path.dirname(im.HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    for name, args in (("pair_groups", [i64]), ("pair_group_begin", [i64, i64]), ("pair_parts", [i64]), ("pair_part_begin", [i64, i64]),
                       ("pair_span_tiles", [i64]), ("pair_span_cap", [])):
        getattr(lib, name).restype = i64
        getattr(lib, name).argtypes = args
    lib.pair_tree32.restype = dbl
    lib.pair_tree32.argtypes = [vp]
    lib.infonce_pair_mirror.restype = ci
    lib.infonce_pair_mirror.argtypes = [vp, vp, i64, i64, dbl, ci, ci, dbl, vp, vp, vp, vp, vp, vp]
    return lib


def run(lib, a, b, tau, positive="scaled", g=None):
    """The mirror on float32 (N, F) arrays: a dict of loss (float64 scalar), rows, z [2, N] float64 (the anchors' list, then the
    samples'), sii [N] float32 and, with the upstream gradient g, ga, gb (N, F) float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape and a.ndim == 2
    n, f = a.shape
    z, rows, loss, sii = np.empty((2, n)), np.empty((2, n)), np.empty(1), np.empty(n, dtype=np.float32)
    ga = np.empty_like(a) if g is not None else None
    gb = np.empty_like(b) if g is not None else None
    rc = lib.infonce_pair_mirror(a.ctypes.data, b.ctypes.data, n, f, float(tau), 1 if positive == "raw" else 0, THREADS,
                                 float(g if g is not None else 0.0), z.ctypes.data, rows.ctypes.data, loss.ctypes.data, sii.ctypes.data,
                                 ga.ctypes.data if g is not None else None, gb.ctypes.data if g is not None else None)
    assert rc == 0, "the mirror refused its arguments"
    return {"loss": loss[0], "rows": rows, "z": z, "sii": sii, "ga": ga, "gb": gb}


def exact_views_fast(n, f, seed=None):
    """The construction of the GPU tests' exact_views without its loop over the rows, for N where that loop is too slow: a_i =
    e_(i mod F); b_j = four entries +-1 in four distinct columns, the columns of every row drawn at once as the first four of a random
    order of the F (the argsort of F uniform numbers), the signs at once.  Not the same draws as exact_views."""
    assert f >= 4
    rng = np.random.RandomState(n + f if seed is None else seed)
    a = np.zeros((n, f), dtype=np.float32)
    a[np.arange(n), np.arange(n) % f] = 1.0
    cols = np.argsort(rng.random_sample((n, f)), axis=1)[:, :4]
    b = np.zeros((n, f), dtype=np.float32)
    b[np.arange(n)[:, None], cols] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), (n, 4))
    return a, b


def restatement(a, b, tau, positive, g=1.0):
    """(loss, ga, gb) of 0.5 * (l(a, b) + l(b, a)) from the float64 restatement of the one-direction loss and its autograd."""
    l1, ga1, gb1 = im.restatement(a, b, tau, positive, g=0.5 * g)
    l2, gb2, ga2 = im.restatement(b, a, tau, positive, g=0.5 * g)
    return 0.5 * (l1 + l2), ga1 + ga2, gb1 + gb2


def two_runs(lib1, a, b, tau, positive, g=1.0):
    """The same from two runs of the existing one-direction mirror (lib1: infonce_mirror.build): a dict as run(), sii of (a, b) and
    of (b, a)."""
    m1 = im.run(lib1, a, b, tau, positive, g=0.5 * g)
    m2 = im.run(lib1, b, a, tau, positive, g=0.5 * g)
    return {"loss": 0.5 * (m1["loss"] + m2["loss"]), "ga": m1["ga"].astype(np.float64) + m2["gb"], "gb": m1["gb"].astype(np.float64) + m2["ga"],
            "sii": m1["sii"], "sii_swapped": m2["sii"], "z": np.stack([m1["z"], m2["z"]])}
