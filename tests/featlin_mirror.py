"""Loader of the feature plan's host mirror (tests/csrc/featlin_mirror.cc around rlap_amd/csrc/rlap_featlin.h, rlap_plan.h and
rlap_spmm.h), shared by tests/test_featlin_cpu.py and the tests/test_gpu_featlin*.py files: the build, both planned calls, the
decoding of a plan buffer into its parts, and the inputs the tests share (the crafted matrix, the four kinds of masks, the dense
float64 reference and the comparison against its bound)."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "csrc", "featlin_mirror.cc")
CHUNK = 256
DIRS = {"forward": (1, 0), "transposed": (0, 1), "both": (1, 1)}
DESC = ("num_nodes", "in_features", "nnz", "chunks_forward", "chunks_transposed", "off_forward", "dir_forward", "rec_forward",
        "off_transposed", "dir_transposed", "rec_transposed", "plan_bytes")
LENGTHS = (0, 1, 255, 256, 257, 513)   # the list lengths around the chunk


class Refused(ValueError):
    pass


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libfeatlin_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    lib = ctypes.CDLL(so)
    i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    for name in ("featlin_chunk", "featlin_max_views", "featlin_magic"):
        getattr(lib, name).restype = ci
    lib.featlin_layout.restype = None
    lib.featlin_layout.argtypes = [i64, i64, i64, ci, ci, vp]
    lib.featlin_count.restype = i64
    lib.featlin_count.argtypes = [vp, ci, i64, i64]
    lib.featlin_build.restype = ci
    lib.featlin_build.argtypes = [vp, ci, i64, i64, i64, ci, ci, vp, i64, vp, vp]
    lib.featlin_apply.restype = ci
    lib.featlin_apply.argtypes = [vp, i64, vp, ci, ci, vp, vp, i64, i64, vp]
    lib.featlin_dir_first.restype = i64
    lib.featlin_dir_first.argtypes = [vp, i64, vp, ci, i64]
    return lib


def layout(lib, N, Fin, nnz, directions="both"):
    out = np.zeros(7, dtype=np.int64)
    f, t = DIRS[directions]
    lib.featlin_layout(N, Fin, nnz, f, t, out.ctypes.data)
    return dict(zip(("off_forward", "off_transposed", "dir_forward", "dir_transposed", "rec_forward", "rec_transposed", "bytes"), out.tolist()))


def _dense(x):
    x = np.ascontiguousarray(x)
    assert x.ndim == 2 and x.dtype in (np.float32, np.float64)
    return x


def count(lib, x):
    x = _dense(x)
    return int(lib.featlin_count(x.ctypes.data, int(x.dtype == np.float32), x.shape[0], x.shape[1]))


def plan(lib, x, directions="both", nnz=None):
    """The plan of the dense matrix x by the mirror: {"buffer": uint8 array, "desc": dict, "info": dict}.  Raises Refused when `nnz`
    is given and is not the matrix's count."""
    x = _dense(x)
    N, Fin = x.shape
    n = count(lib, x) if nnz is None else int(nnz)
    f, t = DIRS[directions]
    buf = np.full(layout(lib, N, Fin, n, directions)["bytes"], 0xA5, dtype=np.uint8)
    desc, info = np.zeros(len(DESC), dtype=np.int64), np.zeros(6, dtype=np.int64)
    rc = lib.featlin_build(x.ctypes.data, int(x.dtype == np.float32), N, Fin, n, f, t, buf.ctypes.data, buf.size, desc.ctypes.data, info.ctypes.data)
    if rc != 0:
        raise Refused(f"feature plan mirror: status {rc}")
    return {"buffer": buf, "desc": dict(zip(DESC, desc.tolist())), "directions": directions,
            "info": dict(zip(("longest_forward", "longest_transposed", "long_lists_forward", "long_lists_transposed"), info[:4].tolist()))}


def _desc_array(desc):
    return np.array([int(desc[k] if isinstance(desc, dict) else getattr(desc, k)) for k in DESC], dtype=np.int64)


def apply(lib, p, w, keep=None, transpose=False, buffer=None):
    """A planned call by the mirror on the plan p (of `plan`), or on `buffer` in place of its own.  Forward: w (Fin, F) gives
    (K, N, F); transposed: w is G (K, N, F) and the result (Fin, F)."""
    w = np.ascontiguousarray(w)
    assert w.dtype in (np.float32, np.float64)
    d = p["desc"]
    N, Fin, F = d["num_nodes"], d["in_features"], w.shape[-1]
    k8 = None if keep is None else np.ascontiguousarray(np.asarray(keep).astype(np.uint8))
    K = 1 if k8 is None else k8.shape[0]
    out = np.full((Fin, F) if transpose else (K, N, F), np.nan, dtype=w.dtype)
    buf = p["buffer"] if buffer is None else np.ascontiguousarray(buffer)
    da = _desc_array(d)
    rc = lib.featlin_apply(buf.ctypes.data, buf.size, da.ctypes.data, int(transpose), int(w.dtype == np.float32), w.ctypes.data,
                           None if k8 is None else k8.ctypes.data, K, F, out.ctypes.data)
    if rc != 0:
        raise Refused(f"feature plan mirror: status {rc}")
    return out


def decode(buffer, desc):
    """The parts of a plan buffer (a uint8 array; `desc` a dict or an rlap_feature_desc) per direction that is there:
    {"forward": {"off", "c", "id", "zero", "dir_slot", "dir_k"}, ...}."""
    buf = np.ascontiguousarray(buffer)
    d = dict(zip(DESC, _desc_array(desc).tolist()))
    out = {}
    for name, slots in (("forward", d["num_nodes"]), ("transposed", d["in_features"])):
        off, dr, rec, ch = d["off_" + name], d["dir_" + name], d["rec_" + name], d["chunks_" + name]
        if off < 0:
            continue
        o = buf[off:off + 8 * (slots + 1)].view(np.int64)
        r = buf[rec:rec + 16 * d["nnz"]].view(np.dtype([("c", np.float64), ("id", np.int32), ("zero", np.int32)]))
        q = buf[dr:dr + 16 * ch].view(np.int64).reshape(-1, 2)
        out[name] = {"off": o.copy(), "c": r["c"].copy(), "id": r["id"].copy(), "zero": r["zero"].copy(), "dir_slot": q[:, 0].copy(), "dir_k": q[:, 1].copy()}
    return out


def same_parts(a, b):
    """Whether two decoded plans hold the same parts, coefficients compared as bits."""
    if sorted(a) != sorted(b):
        return False
    for name in a:
        for key in a[name]:
            x, y = a[name][key], b[name][key]
            if x.shape != y.shape or not np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y):
                return False
    return True


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ shared inputs
def crafted(dtype=np.float32, seed=5):
    """A 520 x 520 matrix whose rows and whose columns have 0, 1, 255, 256, 257 and 513 kept entries (LENGTHS), with a -0.0 (dropped),
    a denormal and a NaN among the rest: row r < 6 has LENGTHS[r] entries in the columns from 6 on, column c < 6 has LENGTHS[c]
    entries in the rows from 6 on, and the corner and everything else is zero."""
    rng = np.random.default_rng(seed)
    x = np.zeros((520, 520), dtype=np.float64)
    for r, n in enumerate(LENGTHS):
        cols = 6 + np.sort(rng.choice(514, size=n, replace=False))
        x[r, cols] = rng.uniform(0.25, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    for c, n in enumerate(LENGTHS):
        rows = 6 + np.sort(rng.choice(514, size=n, replace=False))
        x[rows, c] = rng.uniform(0.25, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)
    x = x.astype(dtype)
    x[0, 1] = -0.0                                     # dropped: row 0 and column 1 stay at 0 and 1 entries
    r5 = np.flatnonzero(x[5])
    x[5, r5[3]] = np.finfo(dtype).smallest_subnormal   # a denormal stays an entry
    return x


def crafted_with_nan(dtype=np.float32, seed=5):
    x = crafted(dtype, seed)
    r4 = np.flatnonzero(x[4])
    x[4, r4[7]] = np.nan                               # a NaN stays an entry (and makes its row and column NaN)
    return x


def random_sparse(N, Fin, per_row, dtype=np.float32, seed=1):
    rng = np.random.default_rng(seed)
    x = np.zeros((N, Fin), dtype=dtype)
    for i in range(N):
        n = min(Fin, int(rng.integers(0, per_row + 1)))
        x[i, rng.choice(Fin, size=n, replace=False)] = rng.uniform(0.1, 1.0, size=n).astype(dtype)
    return x


def masks(kind, K, x, seed=3):
    """(K, Fin) uint8 keep masks: "all", "none", "chunk" (view 0 drops the columns of the first whole chunk of the longest row's
    list; the other views are random), "random"."""
    Fin = x.shape[1]
    rng = np.random.default_rng(seed)
    if kind == "all":
        return np.ones((K, Fin), dtype=np.uint8)
    if kind == "none":
        return np.zeros((K, Fin), dtype=np.uint8)
    keep = (rng.uniform(size=(K, Fin)) < 0.6).astype(np.uint8)
    if kind == "chunk":
        kept = (x.astype(np.float64) != 0.0) | np.isnan(x)
        row = int(np.argmax(kept.sum(1)))
        keep[0, np.flatnonzero(kept[row])[:CHUNK]] = 0
        keep[0, np.flatnonzero(kept[row])[CHUNK:]] = 1
    else:
        keep[:, ::17] *= 3                               # any non-zero byte keeps
    return keep


def reference(x, w, keep, transpose):
    """The dense float64 product and A, the same sum of absolute terms: forward (x * keep[k]) @ W, transposed
    sum_k keep[k][:, None] * (x.T @ G[k])."""
    xd, wd = x.astype(np.float64), w.astype(np.float64)
    K = 1 if keep is None else keep.shape[0]
    kb = np.ones((K, x.shape[1])) if keep is None else (np.asarray(keep) != 0).astype(np.float64)
    if not transpose:
        return np.stack([(xd * kb[k]) @ wd for k in range(K)]), np.stack([(np.abs(xd) * kb[k]) @ np.abs(wd) for k in range(K)])
    ref = sum(kb[k][:, None] * (xd.T @ wd[k]) for k in range(K))
    return ref, sum(kb[k][:, None] * (np.abs(xd).T @ np.abs(wd[k])) for k in range(K))


def within_bound(y, ref, A, factor):
    """|y - ref| <= factor * A (+ 2^-24 (|ref| + bound) for a float32 result), where A is not NaN; `factor` is
    tests/test_gpu_propagate.py's bound_factor(terms of the longest sum, True).  Returns (ok, the worst ratio to the bound)."""
    bound = factor * A
    if y.dtype == np.float32:
        bound = bound + 2.0 ** -24 * (np.abs(ref) + bound)
    sel = ~np.isnan(A)
    err = np.abs(y.astype(np.float64) - ref)[sel]
    bound = bound[sel]
    ok = bool((err <= bound).all())
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return ok, float(ratio.max()) if ratio.size else 0.0
