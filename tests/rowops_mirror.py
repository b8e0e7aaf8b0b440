"""Loader of the row passes' host mirror (tests/csrc/rowops_mirror.cc around rlap_amd/csrc/rlap_rowops.h), the input generator and
the float64 torch restatements of the fused bias-activation-dropout pass and of the layer norm, shared by tests/test_rowops_cpu.py
and the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_rowops.h")
SRC = os.path.join(ROOT, "tests", "csrc", "rowops_mirror.cc")
ACT_RELU, ACT_PRELU, SLOPE_PER_CHANNEL, TRAINING = 1, 2, 4, 8
ACT = {"none": 0, "relu": ACT_RELU, "prelu": ACT_PRELU}
MASK64 = (1 << 64) - 1


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "librowops_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, u64, u32, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p
    lib.rowops_const.restype = i64
    lib.rowops_const.argtypes = [ci]
    lib.rowops_args_ok.restype = ci
    lib.rowops_args_ok.argtypes = [i64, i64, i64, ci, ci, dbl]
    lib.rowops_ln_args_ok.restype = ci
    lib.rowops_ln_args_ok.argtypes = [i64, i64, i64, ci, ci, dbl, dbl]
    lib.rowops_threshold.restype = u32
    lib.rowops_threshold.argtypes = [dbl, ci]
    lib.rowops_scale.restype = dbl
    lib.rowops_scale.argtypes = [u32]
    lib.rowops_split_of.restype = ci
    lib.rowops_split_of.argtypes = [i64, ci]
    lib.rowops_backward_bytes.restype = i64
    lib.rowops_backward_bytes.argtypes = [i64, i64, i64, ci, ci]
    lib.rowops_ln_backward_bytes.restype = i64
    lib.rowops_ln_backward_bytes.argtypes = [i64, i64, i64, ci, ci, ci]
    lib.rowops_ln_lg.restype = ci
    lib.rowops_ln_lg.argtypes = [i64]
    lib.rowops_ln_instance.restype = ci
    lib.rowops_ln_instance.argtypes = [i64]
    lib.rowops_row_sum.restype = dbl
    lib.rowops_row_sum.argtypes = [vp, i64]
    lib.rowops_mask.restype = None
    lib.rowops_mask.argtypes = [i64, i64, i64, dbl, u64, ci, vp]
    lib.rowops_forward.restype = ci
    lib.rowops_forward.argtypes = [vp, i64, i64, i64, vp, vp, dbl, u64, ci, vp]
    lib.rowops_backward.restype = ci
    lib.rowops_backward.argtypes = [vp, vp, i64, i64, i64, vp, vp, dbl, u64, ci, vp, vp, vp]
    lib.rowops_ln_forward.restype = ci
    lib.rowops_ln_forward.argtypes = [vp, i64, i64, i64, vp, vp, vp, dbl, dbl, u64, ci, vp, vp]
    lib.rowops_ln_backward.restype = ci
    lib.rowops_ln_backward.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, dbl, dbl, u64, ci, vp, vp, vp, vp]
    return lib


def constants(lib):
    return {"max_grid": lib.rowops_const(0), "group_waves": lib.rowops_const(1), "max_f": lib.rowops_const(2), "chunk": lib.rowops_const(3),
            "salt": (lib.rowops_const(4) << 32) | lib.rowops_const(5)}


def flags_of(act="none", per_channel=False, training=True):
    return ACT[act] | (SLOPE_PER_CHANNEL if per_channel else 0) | (TRAINING if training else 0)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return None if a is None else a.ctypes.data


def mask(lib, L, n, f, p, seed, flags=TRAINING):
    """The mirror's keep mask (L, n, f), bool."""
    keep = np.empty((L, n, f), dtype=np.uint8)
    lib.rowops_mask(L, n, f, float(p), seed & MASK64, int(flags), keep.ctypes.data)
    return keep.astype(bool)


def forward(lib, x, bias=None, slope=None, p=0.0, seed=0, flags=0):
    x = _f32(x)
    L, n, f = x.shape
    b, s = _f32(bias), _f32(slope)
    y = np.empty_like(x)
    rc = lib.rowops_forward(x.ctypes.data, L, n, f, _p(b), _p(s), float(p), seed & MASK64, int(flags), y.ctypes.data)
    assert rc == 0, "the mirror refused its arguments"
    return y


def backward(lib, x, gy, bias=None, slope=None, p=0.0, seed=0, flags=0, want=("gx", "gbias", "gslope")):
    """The mirror's backward call: a dict of gx, gbias, gslope (the last None without PReLU)."""
    x, gy = _f32(x), _f32(gy)
    L, n, f = x.shape
    b, s = _f32(bias), _f32(slope)
    gx = np.empty_like(x) if "gx" in want else None
    gb = np.empty(f, dtype=np.float32) if "gbias" in want else None
    gs = np.empty(f if flags & SLOPE_PER_CHANNEL else 1, dtype=np.float32) if flags & ACT_PRELU and "gslope" in want else None
    rc = lib.rowops_backward(x.ctypes.data, gy.ctypes.data, L, n, f, _p(b), _p(s), float(p), seed & MASK64, int(flags), _p(gx), _p(gb), _p(gs))
    assert rc == 0, "the mirror refused its arguments"
    return {"gx": gx, "gbias": gb, "gslope": gs}


def ln_forward(lib, x, weight=None, bias=None, slope=None, eps=1e-5, p=0.0, seed=0, flags=0):
    """The mirror's layer norm: (y, stat (L, n, 2) float64: mean, rstd)."""
    x = _f32(x)
    L, n, f = x.shape
    w, b, s = _f32(weight), _f32(bias), _f32(slope)
    y, stat = np.empty_like(x), np.empty((L, n, 2))
    rc = lib.rowops_ln_forward(x.ctypes.data, L, n, f, _p(w), _p(b), _p(s), float(eps), float(p), seed & MASK64, int(flags), y.ctypes.data, stat.ctypes.data)
    assert rc == 0, "the mirror refused its arguments"
    return y, stat


def ln_backward(lib, x, gy, weight=None, bias=None, slope=None, eps=1e-5, p=0.0, seed=0, flags=0):
    x, gy = _f32(x), _f32(gy)
    L, n, f = x.shape
    w, b, s = _f32(weight), _f32(bias), _f32(slope)
    gx, gw, gb = np.empty_like(x), np.empty(f, dtype=np.float32), np.empty(f, dtype=np.float32)
    gs = np.empty(f if flags & SLOPE_PER_CHANNEL else 1, dtype=np.float32) if flags & ACT_PRELU else None
    rc = lib.rowops_ln_backward(x.ctypes.data, gy.ctypes.data, L, n, f, _p(w), _p(b), _p(s), float(eps), float(p), seed & MASK64, int(flags),
                                gx.ctypes.data, gw.ctypes.data, gb.ctypes.data, _p(gs))
    assert rc == 0, "the mirror refused its arguments"
    return {"gx": gx, "gweight": gw, "gbias": gb, "gslope": gs}


def row_sum(lib, terms):
    t = np.ascontiguousarray(terms, dtype=np.float64)
    return lib.rowops_row_sum(t.ctypes.data, len(t))


# ---- the inputs
def inputs(L, n, f, seed):
    """x (L, n, f) float32 with exact +0.0 and -0.0 among its values, one constant row and one row with an outlier a layer; bias,
    weight and a slope per channel (f,); a fixed pseudo-random upstream gy."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((L, n, f))
    x[:, ::3, ::5] = 0.0
    x[:, 1::4, 1::7] = -0.0
    x[:, n // 2, :] = 1.5
    x[:, 0, 0] = 1e3
    out = {"x": x.astype(np.float32), "gy": rng.standard_normal((L, n, f)).astype(np.float32)}
    out["weight"] = (1.0 + 0.5 * rng.standard_normal(f)).astype(np.float32)
    out["bias"] = (0.5 * rng.standard_normal(f)).astype(np.float32)
    out["slope"] = (0.25 + 0.1 * rng.standard_normal(f)).astype(np.float32)
    return out


# ---- torch, restated
def _t64(a, grad=False):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float32)).double().requires_grad_(grad)


def _act(v, act, ts):
    """relu, or prelu with the channels along the LAST dimension (F.prelu takes dimension 1 for them: it is called on the rows as
    (L * N, F))."""
    if act == "relu":
        return torch.relu(v)
    if act == "prelu":
        return torch.nn.functional.prelu(v.reshape(-1, v.shape[-1]), ts).reshape(v.shape)
    return v


def restatement(x, keep, s, gy=None, bias=None, slope=None, act="none"):
    """torch.where(keep, act(x64 + b64) * s, 0) in float64 on float32 inputs, and its gradients of sum(y * gy) by autograd."""
    tx, tb, ts = _t64(x, gy is not None), _t64(bias, gy is not None), _t64(slope, gy is not None)
    v = tx if tb is None else tx + tb
    y = torch.where(torch.from_numpy(keep), _act(v, act, ts) * s, torch.zeros((), dtype=torch.float64))
    out = {"y": y.detach().numpy(), "v": v.detach().numpy()}
    if gy is not None:
        (y * _t64(gy)).sum().backward()
        out.update(gx=tx.grad.numpy(), gbias=None if tb is None else tb.grad.numpy(), gslope=None if ts is None else ts.grad.numpy())
    return out


def ln_restatement(x, keep, s, gy=None, weight=None, bias=None, slope=None, eps=1e-5, post="none"):
    """torch.nn.functional.layer_norm in float64 on float32 inputs, then the activation and the given mask; xh, the normalised
    values, v = xh w + b, and the gradients of sum(y * gy) by autograd."""
    tx, tw, tb, ts = _t64(x, gy is not None), _t64(weight, gy is not None), _t64(bias, gy is not None), _t64(slope, gy is not None)
    f = tx.shape[-1]
    v = torch.nn.functional.layer_norm(tx, (f,), tw, tb, eps)
    with torch.no_grad():
        xh = torch.nn.functional.layer_norm(tx, (f,), None, None, eps)
    y = torch.where(torch.from_numpy(keep), _act(v, post, ts) * s, torch.zeros((), dtype=torch.float64))
    out = {"y": y.detach().numpy(), "xh": xh.numpy(), "v": v.detach().numpy()}
    if gy is not None:
        (y * _t64(gy)).sum().backward()
        out.update(gx=tx.grad.numpy(), gweight=None if tw is None else tw.grad.numpy(), gbias=None if tb is None else tb.grad.numpy(),
                   gslope=None if ts is None else ts.grad.numpy())
    return out
