"""Loader of the per-view batch norm's host mirror (tests/csrc/norm_mirror.cc around rlap_amd/csrc/rlap_norm.h), the input
generator and the float64 torch restatement (torch.nn.functional.batch_norm per layer, relu in front and relu / prelu behind as
flagged), shared by tests/test_norm_cpu.py and the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_norm.h")
SRC = os.path.join(ROOT, "tests", "csrc", "norm_mirror.cc")
PRE_RELU, POST_RELU, POST_PRELU, SLOPE_PER_CHANNEL, EVAL = 1, 2, 4, 8, 16
PRE = {"none": 0, "relu": PRE_RELU}
POST = {"none": 0, "relu": POST_RELU, "prelu": POST_PRELU}


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libnorm_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    lib.norm_const.restype = i64
    lib.norm_const.argtypes = [ci]
    lib.norm_args_ok.restype = ci
    lib.norm_args_ok.argtypes = [i64, i64, i64, ci, ci, ci, dbl, dbl]
    lib.norm_dispatch.restype = None
    lib.norm_dispatch.argtypes = [i64, ci, vp]
    lib.norm_num_items.restype = i64
    lib.norm_num_items.argtypes = [i64, i64, i64, ci]
    lib.norm_item_of.restype = ci
    lib.norm_item_of.argtypes = [i64, ci, i64, i64, i64, ci, vp]
    for name in ("norm_forward_bytes", "norm_backward_bytes"):
        getattr(lib, name).restype = i64
        getattr(lib, name).argtypes = [i64, i64, i64, ci]
    lib.norm_forward.restype = ci
    lib.norm_forward.argtypes = [vp, i64, i64, i64, vp, vp, vp, vp, vp, dbl, dbl, ci, vp, vp]
    lib.norm_backward.restype = ci
    lib.norm_backward.argtypes = [vp, vp, i64, i64, i64, vp, vp, vp, vp, vp, dbl, ci, vp, vp, vp, vp, vp]
    return lib


def constants(lib):
    """The launchers' constants: workgroups of a launch, waves of a workgroup, the largest F, the chunk."""
    return {"max_grid": lib.norm_const(0), "group_waves": lib.norm_const(1), "max_f": lib.norm_const(2), "chunk": lib.norm_const(3)}


def dispatch(lib, f, aligned=True):
    out = (ctypes.c_int64 * 4)()
    lib.norm_dispatch(f, int(aligned), out)
    return {"vec": bool(out[0]), "lanes": out[1], "lg": out[2], "ftiles": out[3]}


def flags_of(pre="none", post="none", per_channel=False, training=True):
    return PRE[pre] | POST[post] | (SLOPE_PER_CHANNEL if per_channel else 0) | (0 if training else EVAL)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _p(a):
    return None if a is None else a.ctypes.data


def forward(lib, x, weight=None, bias=None, slope=None, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, flags=0):
    """The mirror's forward call on x (L, N, F) float32: a dict of y, stat (L, 3, F) float64 (training) and the updated copies of
    the running buffers."""
    x = _f32(x)
    L, n, f = x.shape
    w, b, s = _f32(weight), _f32(bias), _f32(slope)
    rm = None if running_mean is None else _f32(running_mean).copy()
    rv = None if running_var is None else _f32(running_var).copy()
    y, stat = np.empty_like(x), np.zeros((L, 3, f))
    rc = lib.norm_forward(x.ctypes.data, L, n, f, _p(w), _p(b), _p(s), _p(rm), _p(rv), float(momentum), float(eps), int(flags), y.ctypes.data,
                          stat.ctypes.data)
    assert rc == 0, "the mirror refused its arguments"
    return {"y": y, "stat": stat, "running_mean": rm, "running_var": rv}


def backward(lib, x, gy, stat, weight=None, bias=None, slope=None, running_mean=None, running_var=None, eps=1e-5, flags=0):
    """The mirror's backward call: a dict of gx, gweight, gbias, gslope (the last None without PReLU)."""
    x, gy = _f32(x), _f32(gy)
    L, n, f = x.shape
    w, b, s, rm, rv = _f32(weight), _f32(bias), _f32(slope), _f32(running_mean), _f32(running_var)
    gx, gw, gb = np.empty_like(x), np.empty(f, dtype=np.float32), np.empty(f, dtype=np.float32)
    gs = np.empty(f if flags & SLOPE_PER_CHANNEL else 1, dtype=np.float32) if flags & POST_PRELU else None
    stat = np.ascontiguousarray(stat, dtype=np.float64)
    rc = lib.norm_backward(x.ctypes.data, gy.ctypes.data, L, n, f, _p(w), _p(b), _p(s), _p(rm), _p(rv), float(eps), int(flags), stat.ctypes.data,
                           gx.ctypes.data, gw.ctypes.data, gb.ctypes.data, _p(gs))
    assert rc == 0, "the mirror refused its arguments"
    return {"gx": gx, "gweight": gw, "gbias": gb, "gslope": gs}


# ---- the inputs
def inputs(L, n, f, seed):
    """x (L, n, f) float32 whose columns cycle through eight kinds: 0 values with exact +0.0 and -0.0 among them; 1 a constant
    column (1.5); 2 a column of negative values, which pre="relu" empties entirely; 3 an outlier first row (1e3 deviations); 4 to 7
    columns of deviation `sd` around offsets of 0, 10, 100 and 1000 deviations.  Also weight, bias (f,), a slope per channel and a
    fixed pseudo-random upstream gy."""
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((L, n, f))
    for k in range(f):
        kind = k % 8
        if kind == 0:
            x[:, ::3, k] = 0.0
            x[:, 1::5, k] = -0.0
        elif kind == 1:
            x[:, :, k] = 1.5
        elif kind == 2:
            x[:, :, k] = -np.abs(x[:, :, k]) - 0.125
        elif kind == 3:
            x[:, 0, k] = 1e3
        else:
            sd = 0.5 + 0.25 * (k % 3)
            x[:, :, k] = sd * x[:, :, k] + sd * 10.0 ** (kind - 4) * (kind > 4)
    out = {"x": x.astype(np.float32), "gy": rng.standard_normal((L, n, f)).astype(np.float32)}
    out["weight"] = (1.0 + 0.5 * rng.standard_normal(f)).astype(np.float32)
    out["bias"] = (0.5 * rng.standard_normal(f)).astype(np.float32)
    out["slope"] = (0.25 + 0.1 * rng.standard_normal(f)).astype(np.float32)
    out["running_mean"] = (0.3 * rng.standard_normal(f)).astype(np.float32)
    out["running_var"] = (0.5 + rng.random_sample(f)).astype(np.float32)
    return out


# ---- torch, restated
def _t64(a, grad=False):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float32)).double().requires_grad_(grad)


def restatement(x, gy=None, weight=None, bias=None, slope=None, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5,
                pre="none", post="none"):
    """torch.nn.functional.batch_norm per layer in float64 on float32 inputs, F.relu in front and F.relu / F.prelu behind as
    asked: y (L, N, F); xh, the normalised values, and the gradients of sum(y * gy) by autograd when gy is given."""
    tx = _t64(x, gy is not None)
    tw, tb, ts = _t64(weight, gy is not None), _t64(bias, gy is not None), _t64(slope, gy is not None)
    rm, rv = _t64(running_mean), _t64(running_var)
    ys, xhs = [], []
    for l in range(tx.shape[0]):
        u = torch.relu(tx[l]) if pre == "relu" else tx[l]
        v = torch.nn.functional.batch_norm(u, None if training else rm, None if training else rv, tw, tb, training, momentum, eps)
        with torch.no_grad():
            xhs.append(torch.nn.functional.batch_norm(u, None if training else rm, None if training else rv, None, None, training, momentum, eps))
        ys.append(torch.relu(v) if post == "relu" else (torch.nn.functional.prelu(v, ts) if post == "prelu" else v))
    y = torch.stack(ys)
    out = {"y": y.detach().numpy(), "xh": torch.stack(xhs).numpy()}
    if gy is not None:
        (y * _t64(gy)).sum().backward()
        out.update(gx=tx.grad.numpy(), gweight=None if tw is None else tw.grad.numpy(), gbias=None if tb is None else tb.grad.numpy(),
                   gslope=None if ts is None else ts.grad.numpy())
    return out


def torch_buffers(x, running_mean, running_var, momentum=0.1, eps=1e-5, pre="none"):
    """The running buffers after one float64 torch call per layer, in layer order, on float32 buffers: every call reads them as
    float64 and its update is rounded to float32, as a float32 module stores it."""
    rm, rv = running_mean.astype(np.float32), running_var.astype(np.float32)
    for l in range(x.shape[0]):
        u = torch.from_numpy(x[l]).double()
        rm64, rv64 = torch.from_numpy(rm).double(), torch.from_numpy(rv).double()
        torch.nn.functional.batch_norm(torch.relu(u) if pre == "relu" else u, rm64, rv64, None, None, True, momentum, eps)
        rm, rv = rm64.numpy().astype(np.float32), rv64.numpy().astype(np.float32)
    return rm, rv
