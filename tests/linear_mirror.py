"""Loader of the fused dense layer's host mirror (tests/csrc/linear_mirror.cc around rlap_amd/csrc/rlap_linear.h) and the float64
numpy restatement of y = act(x W + b) and its gradients, shared by tests/test_linear_cpu.py and the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_linear.h")
SRC = os.path.join(ROOT, "tests", "csrc", "linear_mirror.cc")
THREADS = 8
WEIGHT_OUT_IN = 1
ACT = {"none": 0, "relu": 1, "elu": 2}


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "liblinear_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, u64, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p
    lib.lin_num_parts.restype = i64
    lib.lin_num_parts.argtypes = [i64, i64, i64]
    lib.lin_part_begin.restype = i64
    lib.lin_part_begin.argtypes = [i64, i64, i64, i64]
    for name in ("lin_feature_tiles", "lin_super_tiles", "lin_row_groups"):
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [i64]
    for name in ("lin_col_waves", "lin_row_tiles", "lin_product_instance", "lin_cross_instance", "lin_flags_ok", "lin_act_ok"):
        getattr(lib, name).restype = ci
        getattr(lib, name).argtypes = [ci]
    lib.lin_product_groups.restype = i64
    lib.lin_product_groups.argtypes = [i64, ci]
    lib.lin_wave_row_tile.restype = i64
    lib.lin_wave_row_tile.argtypes = [i64, ci, ci]
    lib.lin_wave_col_tile.restype = ci
    lib.lin_wave_col_tile.argtypes = [ci, ci, ci]
    lib.lin_pair_groups.restype = ci
    lib.lin_pair_groups.argtypes = [i64, i64]
    lib.lin_alpha_ok.restype = ci
    lib.lin_alpha_ok.argtypes = [dbl]
    lib.lin_vec_ok.restype = ci
    lib.lin_vec_ok.argtypes = [i64, u64]
    lib.lin_mirror.restype = ci
    lib.lin_mirror.argtypes = [vp, vp, vp, i64, i64, i64, ci, dbl, ci, ci, ci, vp]
    lib.lin_mirror_backward.restype = ci
    lib.lin_mirror_backward.argtypes = [vp, vp, vp, vp, i64, i64, i64, ci, dbl, ci, ci, ci, vp, vp, vp]
    return lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _dims(x, w, out_in):
    fin, fout = (w.shape[1], w.shape[0]) if out_in else w.shape
    assert x.shape[-1] == fin
    return int(np.prod(x.shape[:-1])), int(fin), int(fout)


def forward(lib, x, w, b=None, act="none", alpha=1.0, out_in=False, threads=THREADS, pad_tiles=0):
    """The mirror's y, of x's leading shape, on float32 arrays; w is (Fin, Fout), or (Fout, Fin) with out_in."""
    x, w = _f32(x), _f32(w)
    b = None if b is None else _f32(b)
    m, fin, fout = _dims(x, w, out_in)
    y = np.empty(x.shape[:-1] + (fout,), dtype=np.float32)
    rc = lib.lin_mirror(x.ctypes.data, w.ctypes.data, None if b is None else b.ctypes.data, m, fin, fout, ACT[act], float(alpha),
                        WEIGHT_OUT_IN if out_in else 0, int(threads), int(pad_tiles), y.ctypes.data)
    assert rc == 0, "the mirror refused its arguments"
    return y


def backward(lib, x, w, y, gy, act="none", alpha=1.0, out_in=False, threads=THREADS, pad_tiles=0, want=("gx", "gw", "gb")):
    """The mirror's gradients from the stored float32 values: a dict of gx (x's shape), gw (w's shape), gb (Fout,)."""
    x, w, y, gy = _f32(x), _f32(w), _f32(y), _f32(gy)
    m, fin, fout = _dims(x, w, out_in)
    assert y.shape == gy.shape == x.shape[:-1] + (fout,)
    out = {"gx": np.empty_like(x) if "gx" in want else None, "gw": np.empty_like(w) if "gw" in want else None,
           "gb": np.empty(fout, dtype=np.float32) if "gb" in want else None}
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = lib.lin_mirror_backward(x.ctypes.data, w.ctypes.data, y.ctypes.data, gy.ctypes.data, m, fin, fout, ACT[act], float(alpha),
                                 WEIGHT_OUT_IN if out_in else 0, int(threads), int(pad_tiles), ptr(out["gx"]), ptr(out["gw"]), ptr(out["gb"]))
    assert rc == 0, "the mirror refused its arguments"
    return out


def inputs(m, fin, fout, seed, bias=True):
    """x (m, fin), w (fin, fout), b (fout,), gy (m, fout) float32: entries of both signs, so that relu and elu meet both branches,
    and a weight that is far from symmetric."""
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal((m, fin)) + 0.25).astype(np.float32)
    w = (rng.standard_normal((fin, fout)) / np.sqrt(fin) + 0.1 * (np.arange(fout) % 3 - 1)).astype(np.float32)
    b = (0.5 * rng.standard_normal(fout)).astype(np.float32) if bias else None
    gy = rng.standard_normal((m, fout)).astype(np.float32)
    return x, w, b, gy


# ---- the float64 restatement
def act64(v, act, alpha):
    if act == "relu":
        return np.where(v > 0, v, 0.0)
    if act == "elu":
        return np.where(v > 0, v, alpha * np.expm1(np.minimum(v, 0.0)))
    return v


def restatement(x, w, b, act="none", alpha=1.0):
    """(y64, v64, A) on float32 inputs widened to float64: A_io = sum_k |x_ik W_ko| + |b_o|, the scale of the forward bound."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    v = x64 @ w64 + (0.0 if b is None else b.astype(np.float64))
    a = np.abs(x64) @ np.abs(w64) + (0.0 if b is None else np.abs(b.astype(np.float64)))
    return act64(v, act, alpha), v, a


def restatement_backward(x, w, y, gy, act="none", alpha=1.0):
    """Float64 gradients from the STORED float32 y and gy, as the rule takes them: t64 = gy d(y); (gx, gw, gb, Ax, Aw) with the
    scales Ax_ik = sum_o |t_io W_ko| and Aw_ko = sum_i |x_ik t_io|."""
    x64, w64, y64, g64 = (a.astype(np.float64) for a in (x, w, y, gy))
    if act == "relu":
        d = np.where(y64 > 0, 1.0, 0.0)
    elif act == "elu":
        d = np.where(y64 > 0, 1.0, y64 + alpha)
    else:
        d = np.ones_like(y64)
    t = g64 * d
    return t @ w64.T, x64.T @ t, t.sum(0), np.abs(t) @ np.abs(w64).T, np.abs(x64).T @ np.abs(t), t
