"""Loader of the fused CCA-SSG loss's host mirror (tests/csrc/cca_mirror.cc around rlap_amd/csrc/rlap_cca.h) and the float64 torch
restatement of the reference's lines (CCA-SSG/model.py:77-78, CCA-SSG/main.py:111-124), shared by tests/test_cca_cpu.py and the GPU
tests."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_cca.h")
SRC = os.path.join(ROOT, "tests", "csrc", "cca_mirror.cc")
THREADS = 8


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libcca_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    lib.cca_parts.restype = i64
    lib.cca_parts.argtypes = [i64, i64]
    lib.cca_part_begin.restype = i64
    lib.cca_part_begin.argtypes = [i64, i64, i64]
    lib.cca_pair_groups.restype = i64
    lib.cca_pair_groups.argtypes = [i64]
    lib.cca_lambd_ok.restype = ci
    lib.cca_lambd_ok.argtypes = [dbl]
    for name in ("cca_feature_tiles", "cca_super_pairs"):
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [i64]
    for name in ("cca_gram_instance", "cca_zr_instance"):
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [ci]
    lib.cca_mirror.restype = ci
    lib.cca_mirror.argtypes = [vp, vp, i64, i64, dbl, i64, ci, ci, dbl, vp, vp, vp, vp, vp]
    return lib


def run(lib, a, b, lambd, g=None, block=32, threads=THREADS, pad_tiles=0):
    """The mirror on float32 (N, F) arrays: a dict of terms [4] float64 (loss, inv, dec1, dec2), colstat [4 F] float64 (mean1, sd1,
    mean2, sd2), gram (2, F, F) float32 and, with the upstream gradient g, ga, gb (N, F) float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape and a.ndim == 2
    n, f = a.shape
    terms, colstat, gram = np.empty(4), np.empty(4 * f), np.empty((2, f, f), dtype=np.float32)
    ga = np.empty_like(a) if g is not None else None
    gb = np.empty_like(b) if g is not None else None
    rc = lib.cca_mirror(a.ctypes.data, b.ctypes.data, n, f, float(lambd), int(block), int(threads), int(pad_tiles),
                        float(g if g is not None else 0.0), terms.ctypes.data, colstat.ctypes.data, gram.ctypes.data,
                        ga.ctypes.data if g is not None else None, gb.ctypes.data if g is not None else None)
    assert rc == 0, "the mirror refused its arguments"
    return {"terms": terms, "loss": terms[0], "inv": terms[1], "dec1": terms[2], "dec2": terms[3], "colstat": colstat, "gram": gram,
            "ga": ga, "gb": gb}


def views(n, f, seed):
    """Two correlated float32 views, b = 0.3 a + noise, with column means that are not zero, so that the centring matters."""
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((n, f)) + 0.5 + 0.01 * np.arange(f)
    b = 0.3 * a + rng.standard_normal((n, f)) - 0.25
    return a.astype(np.float32), b.astype(np.float32)


# ---- the reference's lines, restated in torch
def cca_terms(h1, h2, lambd):
    """(loss, inv, dec1, dec2) of CCA-SSG/model.py:77-78 and CCA-SSG/main.py:111-124 in the dtype of h1."""
    z1 = (h1 - h1.mean(0)) / h1.std(0)
    z2 = (h2 - h2.mean(0)) / h2.std(0)
    n = h1.shape[0]
    c = torch.mm(z1.T, z2)
    c1 = torch.mm(z1.T, z1)
    c2 = torch.mm(z2.T, z2)
    c = c / n
    c1 = c1 / n
    c2 = c2 / n
    loss_inv = -torch.diagonal(c).sum()
    iden = torch.eye(c.shape[0], dtype=h1.dtype, device=h1.device)
    loss_dec1 = (iden - c1).pow(2).sum()
    loss_dec2 = (iden - c2).pow(2).sum()
    return loss_inv + lambd * (loss_dec1 + loss_dec2), loss_inv, loss_dec1, loss_dec2


def restatement(a, b, lambd, g=1.0):
    """(terms [4], ga, gb) of the float64 restatement on float32 inputs (numpy), the gradients by autograd with the upstream g."""
    ta = torch.from_numpy(np.asarray(a, dtype=np.float32)).double().requires_grad_(True)
    tb = torch.from_numpy(np.asarray(b, dtype=np.float32)).double().requires_grad_(True)
    terms = cca_terms(ta, tb, lambd)
    terms[0].backward(torch.tensor(float(g), dtype=torch.float64))
    return np.array([float(t.detach()) for t in terms]), ta.grad.numpy(), tb.grad.numpy()
