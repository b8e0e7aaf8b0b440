"""Loader of the fused Barlow Twins loss's host mirror (tests/csrc/bt_mirror.cc around rlap_amd/csrc/rlap_bt.h) and the float64
torch restatement of the published bt_loss (PyGCL's L.BarlowTwins; the package is not pinned), shared by
tests/test_bt_cpu.py and the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_bt.h")
SRC = os.path.join(ROOT, "tests", "csrc", "bt_mirror.cc")
THREADS = 8
NO_STANDARDIZE = 1


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libbt_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    lib.bt_parts.restype = i64
    lib.bt_parts.argtypes = [i64, i64]
    lib.bt_part_begin.restype = i64
    lib.bt_part_begin.argtypes = [i64, i64, i64]
    lib.bt_pair_groups.restype = i64
    lib.bt_pair_groups.argtypes = [i64]
    for name in ("bt_row_groups", "bt_feature_tiles"):
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [i64]
    for name in ("bt_lambd_ok", "bt_eps_ok"):
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [dbl]
    for name in ("bt_flags_ok", "bt_cross_instance", "bt_zr_instance"):
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [ci]
    lib.bt_mirror.restype = ci
    lib.bt_mirror.argtypes = [vp, vp, i64, i64, dbl, dbl, ci, i64, ci, ci, dbl, vp, vp, vp, vp, vp, vp]
    return lib


def lambd_of(lambd, f):
    return 1.0 / f if lambd is None else float(lambd)


def run(lib, a, b, lambd=None, eps=1e-15, standardize=True, g=None, block=32, threads=THREADS, pad_tiles=0):
    """The mirror on float32 (N, F) arrays: a dict of terms [3] float64 (loss, on, off), colstat [4 F] float64 (mean1, sd1, mean2,
    sd2; NaN-filled and untouched without the standardisation), cross (F, F) float32, z (2, N, F) float32 and, with the upstream
    gradient g, ga, gb (N, F) float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape and a.ndim == 2
    n, f = a.shape
    terms, colstat, cross = np.empty(3), np.full(4 * f, np.nan), np.empty((f, f), dtype=np.float32)
    z = np.empty((2, n, f), dtype=np.float32)
    ga = np.empty_like(a) if g is not None else None
    gb = np.empty_like(b) if g is not None else None
    rc = lib.bt_mirror(a.ctypes.data, b.ctypes.data, n, f, lambd_of(lambd, f), float(eps), 0 if standardize else NO_STANDARDIZE, int(block),
                       int(threads), int(pad_tiles), float(g if g is not None else 0.0), terms.ctypes.data, colstat.ctypes.data,
                       cross.ctypes.data, z.ctypes.data, ga.ctypes.data if g is not None else None, gb.ctypes.data if g is not None else None)
    assert rc == 0, "the mirror refused its arguments"
    return {"terms": terms, "loss": terms[0], "on": terms[1], "off": terms[2], "colstat": colstat, "cross": cross, "z": z, "ga": ga, "gb": gb}


def views(n, f, seed):
    """Two float32 views with column means that are not zero: a = randn + 0.5, b = 0.6 roll(a, -1, axis=1) + 0.4 randn + 1.  Column
    k of b follows column k + 1 of a, so c[k + 1, k] is large and c[k, k + 1] is not: a transposed or triangle-only kernel cannot
    pass."""
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((n, f)) + 0.5
    b = 0.6 * np.roll(a, -1, axis=1) + 0.4 * rng.standard_normal((n, f)) + 1.0
    return a.astype(np.float32), b.astype(np.float32)


# ---- the published loss, restated in torch
def bt_cross(h1, h2, eps=1e-15, standardize=True):
    if standardize:
        h1 = (h1 - h1.mean(0)) / (h1.std(0) + eps)
        h2 = (h2 - h2.mean(0)) / (h2.std(0) + eps)
    return torch.mm(h1.T, h2) / h1.shape[0]


def bt_terms(h1, h2, lambd=None, eps=1e-15, standardize=True):
    """(loss, on, off) of bt_loss in the dtype of h1."""
    c = bt_cross(h1, h2, eps, standardize)
    f = c.shape[0]
    lambd = lambd_of(lambd, f)
    off_mask = ~torch.eye(f, dtype=torch.bool, device=c.device)
    on = (1 - c.diagonal()).pow(2).sum()
    off = c[off_mask].pow(2).sum()
    return on + lambd * off, on, off


def restatement(a, b, lambd=None, eps=1e-15, standardize=True, g=1.0):
    """(terms [3], ga, gb, c) of the float64 restatement on float32 inputs (numpy), the gradients by autograd with the upstream g."""
    ta = torch.from_numpy(np.asarray(a, dtype=np.float32)).double().requires_grad_(True)
    tb = torch.from_numpy(np.asarray(b, dtype=np.float32)).double().requires_grad_(True)
    terms = bt_terms(ta, tb, lambd, eps, standardize)
    terms[0].backward(torch.tensor(float(g), dtype=torch.float64))
    with torch.no_grad():
        c = bt_cross(ta, tb, eps, standardize).numpy()
    return np.array([float(t.detach()) for t in terms]), ta.grad.numpy(), tb.grad.numpy(), c
