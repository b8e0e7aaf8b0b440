"""Loader of the fused InfoNCE loss's host mirror (tests/csrc/infonce_mirror.cc around rlap_amd/csrc/rlap_infonce.h) and the float64
torch restatement of the reference's two losses, shared by tests/test_infonce_cpu.py and the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_infonce.h")
SRC = os.path.join(ROOT, "tests", "csrc", "infonce_mirror.cc")
THREADS = 8


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libinfonce_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp, flt = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    lib.infonce_expw.restype = flt
    lib.infonce_expw.argtypes = [flt]
    lib.infonce_expw_many.restype = None
    lib.infonce_expw_many.argtypes = [vp, i64, vp]
    lib.infonce_parts.restype = i64
    lib.infonce_parts.argtypes = [i64]
    lib.infonce_part_begin.restype = i64
    lib.infonce_part_begin.argtypes = [i64, i64]
    lib.infonce_reg_row.restype = ci
    lib.infonce_reg_row.argtypes = [ci, ci]
    lib.infonce_tau_ok.restype = ci
    lib.infonce_tau_ok.argtypes = [dbl]
    lib.infonce_feature_tiles.restype = ci
    lib.infonce_feature_tiles.argtypes = [i64]
    lib.infonce_main_instance.restype = ci
    lib.infonce_main_instance.argtypes = [ci]
    lib.infonce_mirror.restype = ci
    lib.infonce_mirror.argtypes = [vp, vp, i64, i64, dbl, ci, i64, ci, dbl, vp, vp, vp, vp, vp, vp]
    return lib


def expw(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    lib.infonce_expw_many(x.ctypes.data, x.size, y.ctypes.data)
    return y


def run(lib, a, b, tau, positive="scaled", g=None, block_rows=32):
    """The mirror on float32 (N, F) arrays: a dict of loss (float64 scalar), rows, z [N] float64, sii [N] float32 and, with the upstream
    gradient g, ga, gb (N, F) float32."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert a.shape == b.shape and a.ndim == 2
    n, f = a.shape
    z, rows, loss, sii = np.empty(n), np.empty(n), np.empty(1), np.empty(n, dtype=np.float32)
    ga = np.empty_like(a) if g is not None else None
    gb = np.empty_like(b) if g is not None else None
    rc = lib.infonce_mirror(a.ctypes.data, b.ctypes.data, n, f, float(tau), 1 if positive == "raw" else 0, int(block_rows), THREADS,
                            float(g if g is not None else 0.0), z.ctypes.data, rows.ctypes.data, loss.ctypes.data, sii.ctypes.data,
                            ga.ctypes.data if g is not None else None, gb.ctypes.data if g is not None else None)
    assert rc == 0, "the mirror refused its arguments"
    return {"loss": loss[0], "rows": rows, "z": z, "sii": sii, "ga": ga, "gb": gb}


# ---- the reference's losses, restated in float64 torch (scripts/node_shared.py: _similarity, InfoNCE.compute with all-ones masks but a
# diagonal positive mask, InfoNCEBatched.compute)
def similarity(h1, h2):
    return torch.nn.functional.normalize(h1) @ torch.nn.functional.normalize(h2).t()


def info_nce_scaled(anchor, sample, tau):
    """GCL's InfoNCE: the positive mask is the identity, positives and negatives together cover every column."""
    n = anchor.shape[0]
    pos = torch.eye(n, dtype=anchor.dtype, device=anchor.device)
    sim = similarity(anchor, sample) / tau
    exp_sim = torch.exp(sim) * torch.ones_like(sim)
    log_prob = sim - torch.log(exp_sim.sum(dim=1, keepdim=True))
    loss = (log_prob * pos).sum(dim=1) / pos.sum(dim=1)
    return -loss.mean()


def info_nce_raw_batched(anchor, sample, tau, batch_size=1024):
    """The reference's InfoNCEBatched: blocks of batch_size anchor rows; the positive term is the similarity itself, not divided by tau."""
    n = anchor.shape[0]
    pos = torch.eye(n, dtype=anchor.dtype, device=anchor.device)
    losses = []
    for s in range(0, n, batch_size):
        sim = similarity(anchor[s:s + batch_size], sample)
        log_prob = sim - torch.log(torch.exp(sim / tau).sum(dim=1, keepdim=True))
        losses.append((log_prob * pos[s:s + batch_size]).sum(dim=1))
    return -torch.cat(losses).mean()


def restatement(a, b, tau, positive, g=1.0):
    """(loss, ga, gb) of the float64 restatement on float32 inputs (numpy), the gradients by autograd with the upstream gradient g."""
    ta = torch.from_numpy(np.asarray(a, dtype=np.float32)).double().requires_grad_(True)
    tb = torch.from_numpy(np.asarray(b, dtype=np.float32)).double().requires_grad_(True)
    loss = info_nce_raw_batched(ta, tb, tau) if positive == "raw" else info_nce_scaled(ta, tb, tau)
    loss.backward(torch.tensor(float(g), dtype=torch.float64))
    return float(loss.detach()), ta.grad.numpy(), tb.grad.numpy()
