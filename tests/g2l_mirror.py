"""Loader of the graph-to-local losses' host mirror (tests/csrc/g2l_mirror.cc around rlap_amd/csrc/rlap_g2l.h) and the float64 torch
restatement of the reference's two losses, shared by tests/test_g2l_cpu.py and the GPU tests."""
import ctypes
import math
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_g2l.h")
SRC = os.path.join(ROOT, "tests", "csrc", "g2l_mirror.cc")
THREADS = 8
JSD_FORWARD, JSD_BACKWARD, BOOT_FORWARD, BOOT_BACKWARD = 0, 1, 2, 3   # g2l::Call


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libg2l_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp, flt = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_float
    for name in ("g2l_pos_term", "g2l_neg_term"):
        getattr(lib, name).restype = dbl
        getattr(lib, name).argtypes = [flt]
    lib.g2l_sigma.restype = flt
    lib.g2l_sigma.argtypes = [flt]
    lib.g2l_parts.restype = i64
    lib.g2l_parts.argtypes = [i64, i64, i64]
    lib.g2l_part_begin.restype = i64
    lib.g2l_part_begin.argtypes = [i64, i64, i64, i64]
    lib.g2l_arena_bytes.restype = i64
    lib.g2l_arena_bytes.argtypes = [ci, i64, i64, i64]
    lib.g2l_graph_of.restype = i64
    lib.g2l_graph_of.argtypes = [vp, i64, i64, i64]
    lib.g2l_num_neg.restype = i64
    lib.g2l_num_neg.argtypes = [i64, i64]
    lib.g2l_feature_tiles.restype = ci
    lib.g2l_feature_tiles.argtypes = [i64]
    lib.g2l_main_instance.restype = ci
    lib.g2l_main_instance.argtypes = [ci]
    lib.g2l_vec_rows.restype = ci
    lib.g2l_vec_rows.argtypes = [i64]
    lib.g2l_vec_blocks.restype = i64
    lib.g2l_vec_blocks.argtypes = [i64, i64]
    lib.g2l_jsd_mirror.restype = ci
    lib.g2l_jsd_mirror.argtypes = [vp, vp, vp, i64, i64, vp, i64, i64, ci, dbl, ci, vp, vp, vp, vp, vp]
    lib.g2l_bootstrap_mirror.restype = ci
    lib.g2l_bootstrap_mirror.argtypes = [vp, vp, i64, i64, vp, i64, i64, ci, dbl, ci, vp, vp, vp]
    return lib


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


def _table(node_ptr, n):
    t = np.ascontiguousarray([0, n] if node_ptr is None else node_ptr, dtype=np.int64)
    assert t.ndim == 1 and t.size >= 2
    return t


def run_jsd(lib, h, g, node_ptr=None, neg=None, gup=None, block_rows=32):
    """The mirror on float32 arrays: a dict of loss (float64 scalar), pos, neg [N] float64 and, with the upstream gradient gup, gh,
    gneg (None without neg), gg float32."""
    h, g = _f32(h), _f32(g)
    neg = _f32(neg) if neg is not None else None
    n, f = h.shape
    t = _table(node_ptr, n)
    G = t.size - 1
    assert g.shape == (G, f)
    rows, loss = np.empty(2 * n), np.empty(1)
    grad = gup is not None
    gh = np.empty_like(h) if grad else None
    gneg = np.empty_like(h) if grad and neg is not None else None
    gg = np.empty_like(g) if grad else None
    p = lambda a: a.ctypes.data if a is not None else None
    rc = lib.g2l_jsd_mirror(p(h), p(neg), p(g), n, f, p(t), G, int(block_rows), THREADS, float(gup if grad else 0.0), int(grad),
                            p(rows), p(loss), p(gh), p(gneg), p(gg))
    assert rc == 0, "the mirror refused its arguments"
    return {"loss": loss[0], "pos": rows[:n].copy(), "neg": rows[n:].copy(), "gh": gh, "gneg": gneg, "gg": gg}


def run_bootstrap(lib, h, g, node_ptr=None, gup=None, block_rows=32):
    """The mirror on float32 arrays: a dict of loss (float64 scalar), c [N] float64 and, with the upstream gradient gup, gh float32."""
    h, g = _f32(h), _f32(g)
    n, f = h.shape
    t = _table(node_ptr, n)
    G = t.size - 1
    assert g.shape == (G, f)
    rows, loss = np.empty(n), np.empty(1)
    grad = gup is not None
    gh = np.empty_like(h) if grad else None
    rc = lib.g2l_bootstrap_mirror(h.ctypes.data, g.ctypes.data, n, f, t.ctypes.data, G, int(block_rows), THREADS, float(gup if grad else 0.0),
                                  int(grad), rows.ctypes.data, loss.ctypes.data, gh.ctypes.data if grad else None)
    assert rc == 0, "the mirror refused its arguments"
    return {"loss": loss[0], "c": rows, "gh": gh}


def table(n, g, kind="even", seed=0):
    """A node_ptr of g graphs over n nodes: "even" -- near-equal graphs; "empty" -- random cuts with empty graphs at the front, in
    the middle and at the end (g >= 4); "one" -- graph g // 2 holds every node."""
    if kind == "even":
        return np.array([(n * j) // g for j in range(g + 1)], dtype=np.int64)
    if kind == "one":
        return np.array([0] * (g // 2 + 1) + [n] * (g - g // 2), dtype=np.int64)
    assert kind == "empty" and g >= 4
    rng = np.random.RandomState(seed + 31 * n + g)
    live = g - 3
    cuts = sorted(rng.randint(0, n + 1, size=live - 1).tolist())
    b = [0] + cuts + [n]                                                      # `live` graphs
    mid = len(b) // 2
    t = np.array([0] + b[:mid + 1] + [b[mid]] + b[mid + 1:] + [n], dtype=np.int64)   # an empty graph at the front, in the middle, at the end
    assert t.size == g + 1 and t[0] == 0 and t[-1] == n and (np.diff(t) >= 0).all()
    return t


def batch_of(node_ptr, n):
    t = np.asarray(node_ptr, dtype=np.int64)
    return np.repeat(np.arange(t.size - 1), np.diff(t))


# ---- the reference's losses, restated in float64 torch.  JSD.compute is scripts/node_dedicated.py's; the masks are those of PyGCL's
# published CrossScaleSampler (anchor = the summaries, sample = the nodes; one graph: sample = [h; neg], the positives the first N
# columns, the negatives the last N); BootstrapLatent and BootstrapContrast's G2L mode are PyGCL's as published.
def jsd_compute(anchor, sample, pos_mask, neg_mask):
    num_neg = neg_mask.int().sum()
    num_pos = pos_mask.int().sum()
    similarity = anchor @ sample.t()
    e_pos = (math.log(2) - torch.nn.functional.softplus(-similarity * pos_mask)).sum() / num_pos
    neg_sim = similarity * neg_mask
    e_neg = (torch.nn.functional.softplus(-neg_sim) + neg_sim - math.log(2)).sum() / num_neg
    return e_neg - e_pos


def jsd_g2l(h, g, node_ptr=None, neg=None):
    n = h.shape[0]
    if neg is not None:
        sample = torch.cat([h, neg], dim=0)
        pos = torch.cat([torch.ones(1, n, dtype=h.dtype), torch.zeros(1, n, dtype=h.dtype)], dim=1)
        return jsd_compute(g, sample, pos, 1.0 - pos)
    batch = torch.from_numpy(batch_of(node_ptr, n))
    pos = torch.zeros(g.shape[0], n, dtype=h.dtype)
    pos[batch, torch.arange(n)] = 1.0
    return jsd_compute(g, h, pos, 1.0 - pos)


def bootstrap_g2l(h, g, node_ptr=None):
    n = h.shape[0]
    batch = torch.from_numpy(batch_of([0, n] if node_ptr is None else node_ptr, n))
    pos = torch.zeros(g.shape[0], n, dtype=h.dtype)
    pos[batch, torch.arange(n)] = 1.0
    anchor = torch.nn.functional.normalize(g, dim=-1, p=2)
    sample = torch.nn.functional.normalize(h, dim=-1, p=2)
    similarity = anchor @ sample.t()
    return (similarity * pos).sum(dim=-1).mean()


def restatement(kind, h, g, node_ptr=None, neg=None, gup=1.0):
    """(loss, gh, gneg, gg) of the float64 restatement on float32 inputs (numpy), the gradients by autograd with the upstream
    gradient gup; the bootstrap's targets are detached (gg None)."""
    th = torch.from_numpy(_f32(h)).double().requires_grad_(True)
    tg = torch.from_numpy(_f32(g)).double().requires_grad_(kind == "jsd")
    tn = torch.from_numpy(_f32(neg)).double().requires_grad_(True) if neg is not None else None
    loss = jsd_g2l(th, tg, node_ptr, tn) if kind == "jsd" else bootstrap_g2l(th, tg.detach(), node_ptr)
    loss.backward(torch.tensor(float(gup), dtype=torch.float64))
    return (float(loss.detach()), th.grad.numpy(), tn.grad.numpy() if tn is not None else None, tg.grad.numpy() if kind == "jsd" else None)
