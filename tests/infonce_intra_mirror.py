"""Loader of the host mirror of the InfoNCE calls with intraview negatives (tests/csrc/infonce_intra_mirror.cc around
rlap_amd/csrc/rlap_infonce.h) and the float64 torch restatement of the reference's two losses under the sampler with
intraview_negs=True, shared by tests/test_infonce_intra_cpu.py and the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np
import torch

import infonce_mirror as im

ROOT = im.ROOT
SRC = os.path.join(ROOT, "tests", "csrc", "infonce_intra_mirror.cc")
THREADS = 8
VARIANTS = {"masked": 1, "all": 2}


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libinfonce_intra_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I", os.path.dirname(im.HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    lib.intra_ok.restype = ci
    lib.intra_ok.argtypes = [ci]
    lib.intra_member.restype = ci
    lib.intra_member.argtypes = [ci, i64, i64]
    lib.intra_z_parts.restype = i64
    lib.intra_z_parts.argtypes = [i64]
    for name in ("infonce_intra_mirror", "infonce_pair_intra_mirror"):
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [vp, vp, i64, i64, dbl, ci, ci, i64, ci, dbl, vp, vp, vp, vp, vp, vp]
    return lib


def run(lib, a, b, tau, positive="scaled", intraview="masked", g=None, pair=False, block_rows=32):
    """The mirror on float32 (N, F) arrays: a dict of loss (float64 scalar), rows, z float64 ([N]; the pair: [2, N], the anchors' list,
    then the samples'), sii [N] float32 and, with the upstream gradient g, ga, gb (N, F) float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape and a.ndim == 2
    n, f = a.shape
    lists = (2, n) if pair else (n,)
    z, rows, loss, sii = np.empty(lists), np.empty(lists), np.empty(1), np.empty(n, dtype=np.float32)
    ga = np.empty_like(a) if g is not None else None
    gb = np.empty_like(b) if g is not None else None
    fn = lib.infonce_pair_intra_mirror if pair else lib.infonce_intra_mirror
    rc = fn(a.ctypes.data, b.ctypes.data, n, f, float(tau), 1 if positive == "raw" else 0, VARIANTS[intraview], int(block_rows), THREADS,
            float(g if g is not None else 0.0), z.ctypes.data, rows.ctypes.data, loss.ctypes.data, sii.ctypes.data,
            ga.ctypes.data if g is not None else None, gb.ctypes.data if g is not None else None)
    assert rc == 0, "the mirror refused its arguments"
    return {"loss": loss[0], "rows": rows, "z": z, "sii": sii, "ga": ga, "gb": gb}


# ---- the reference under the sampler with intraview_negs=True, restated in float64 torch: the sample becomes the (2N, F)
# concatenation of the sample and the anchor, the positive mask gains N zero columns, the negative mask gains 1 - I.  GCL's InfoNCE
# multiplies exp(sim) by pos_mask + neg_mask ("masked": the anchor's own row drops out); the reference's InfoNCEBatched never reads the
# negative mask ("all": it stays in).  `positive` is the first term of either: sim / tau ("scaled") or sim ("raw").
def one_direction(anchor, sample, tau, positive, intraview):
    n = anchor.shape[0]
    eye = torch.eye(n, dtype=anchor.dtype)
    both = torch.cat([sample, anchor], dim=0)
    pos = torch.cat([eye, torch.zeros_like(eye)], dim=1)
    neg = torch.cat([1.0 - eye, 1.0 - eye], dim=1)
    sim = im.similarity(anchor, both)
    weight = pos + neg if intraview == "masked" else torch.ones_like(sim)
    first = sim if positive == "raw" else sim / tau
    log_prob = first - torch.log((torch.exp(sim / tau) * weight).sum(dim=1, keepdim=True))
    return -((log_prob * pos).sum(dim=1) / pos.sum(dim=1)).mean()


def restatement(a, b, tau, positive, intraview, g=1.0, pair=False):
    """(loss, ga, gb) of the float64 restatement on float32 inputs (numpy), the gradients by autograd with the upstream gradient g;
    the pair is 0.5 * (l(a, b) + l(b, a))."""
    ta = torch.from_numpy(np.asarray(a, dtype=np.float32)).double().requires_grad_(True)
    tb = torch.from_numpy(np.asarray(b, dtype=np.float32)).double().requires_grad_(True)
    loss = one_direction(ta, tb, tau, positive, intraview)
    if pair:
        loss = 0.5 * (loss + one_direction(tb, ta, tau, positive, intraview))
    loss.backward(torch.tensor(float(g), dtype=torch.float64))
    return float(loss.detach()), ta.grad.numpy(), tb.grad.numpy()


def exact_views(n, f, seed=None):
    """Rows that are signed unit vectors, so that every similarity is 0 or +-1 and every sum is exact: a_i = +-e_(i mod f); b_j =
    +-e_(pi(j) mod f) for a random order pi -- b is not a, and S^ab is not symmetric, so a misplaced or transposed diagonal mask
    changes Z by a whole term."""
    rng = np.random.RandomState(n + 7 * f if seed is None else seed)
    a = np.zeros((n, f), dtype=np.float32)
    b = np.zeros((n, f), dtype=np.float32)
    a[np.arange(n), np.arange(n) % f] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n)
    b[np.arange(n), rng.permutation(n) % f] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), n)
    return a, b
