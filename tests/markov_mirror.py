"""Loader of the Markov diffusion's host mirror (tests/csrc/markov_mirror.cc around rlap_amd/csrc/rlap_markov.h), shared by
tests/test_markov_cpu.py and the tests/test_gpu_markov*.py files, and the dense restatement of the contract in numpy float64 in the
published loop's order (z, t, one product per round).  `run` is one segment on the host, `run_call` a whole call."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "csrc", "markov_mirror.cc")
MAIN = os.path.join(ROOT, "tests", "csrc", "markov_main.cc")
STATUS = {3: "a malformed argument", 5: "a row id without a column", 12: "a column id in two runs of rows"}


class Refused(ValueError):
    def __init__(self, status):
        super().__init__(f"markov mirror: status {status} ({STATUS.get(status, '?')})")
        self.status = status


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libmarkov_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    lib = ctypes.CDLL(so)
    i64, ci, vp, dbl = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    lib.markov_max_order.restype = ci
    lib.markov_final_copy.restype = ci
    lib.markov_final_copy.argtypes = [ci]
    lib.markov_valid.restype = ci
    lib.markov_valid.argtypes = [dbl, ci, dbl]
    lib.markov_run.restype = i64
    lib.markov_run.argtypes = [vp, i64, ci, ci, ci, dbl, ci, dbl, vp, i64]
    lib.markov_fetch.restype = None
    lib.markov_fetch.argtypes = [vp, vp]
    return lib


def run(lib, sc, alpha=0.2, order=16, eps=1e-4, weighted=True, self_loop=True, zero_ok=False, tiles=None):
    """One segment by the mirror: (raw, norm), the kept rows [i, j, value] before and after normalisation, (P, 3) float64 each.
    `tiles`: the source tiles (64 consecutive columns in input order) to compute -- then only the pairs whose smaller id's column
    was computed come back, and `norm` is not meaningful."""
    sc = np.ascontiguousarray(sc, dtype=np.float64).reshape(-1, 3)
    tl = None if tiles is None else np.ascontiguousarray(tiles, dtype=np.int64)
    P = lib.markov_run(sc.ctypes.data if sc.size else None, sc.shape[0], int(weighted), int(self_loop), int(zero_ok), float(alpha),
                       int(order), float(eps), None if tl is None else tl.ctypes.data, -1 if tl is None else tl.size)
    if P < 0:
        raise Refused(-P)
    raw, norm = np.empty((P, 3)), np.empty((P, 3))
    if P:
        lib.markov_fetch(raw.ctypes.data, norm.ctypes.data)
    return raw, norm


def run_call(lib, sc, ptr, normalize=False, **kw):
    """A whole call: every segment by `run`, stacked -- (out (P, 3), mptr (S + 1,)), the layout of ops.snapshot_markov."""
    sc = np.asarray(sc, dtype=np.float64).reshape(-1, 3)
    parts, mptr = [], [0]
    for s in range(len(ptr) - 1):
        raw, norm = run(lib, sc[ptr[s]:ptr[s + 1]], **kw)
        parts.append(norm if normalize else raw)
        mptr.append(mptr[-1] + parts[-1].shape[0])
    return (np.concatenate(parts) if parts else np.empty((0, 3))), np.asarray(mptr, dtype=np.int64)


def dense(sc, alpha=0.2, order=16, weighted=True, self_loop=True):
    """(sorted ids, M before the threshold) of one segment's rows [i, j, w] in numpy float64, in the published loop's order:
    z = Â; t = Â; `order` times: t = beta Â t, z += t; z /= order; z += alpha Â; transposed."""
    sc = np.asarray(sc, dtype=np.float64).reshape(-1, 3)
    nodes = np.unique(sc[:, :2].astype(np.int64))
    k = len(nodes)
    A = np.zeros((k, k))
    r = np.searchsorted(nodes, sc[:, 0].astype(np.int64))
    c = np.searchsorted(nodes, sc[:, 1].astype(np.int64))
    np.add.at(A, (r, c), sc[:, 2] if weighted else 1.0)
    if self_loop:
        A += np.eye(k)
    d = A.sum(1)
    dinv = np.where(d > 0, np.maximum(d, 1e-300) ** -0.5, 0.0)
    ah = dinv[:, None] * A * dinv[None, :]
    z, t = ah.copy(), ah.copy()
    for _ in range(order):
        t = (1.0 - alpha) * (ah @ t)
        z = z + t
    z = z / order
    z = z + alpha * ah
    return nodes, z.T.copy()


def threshold(M, eps, normalize=False):
    """The entries >= eps of M, then (normalize) D^-1/2 . D^-1/2 with D the row sums of what was kept."""
    Z = np.where(M >= eps, M, 0.0)
    if normalize:
        d = Z.sum(1)
        di = np.where(d > 0, np.maximum(d, 1e-300) ** -0.5, 0.0)
        Z = di[:, None] * Z * di[None, :]
    return Z


def to_dense(rows, nodes):
    """(values, pattern) of rows [i, j, value] as dense (k, k) arrays over the sorted ids `nodes`; every (i, j) occurs once."""
    rows = np.asarray(rows).reshape(-1, 3)
    k = len(nodes)
    i = np.searchsorted(nodes, rows[:, 0].astype(np.int64))
    j = np.searchsorted(nodes, rows[:, 1].astype(np.int64))
    assert i.size == 0 or (i.max() < k and j.max() < k)
    assert np.array_equal(nodes[i], rows[:, 0]) and np.array_equal(nodes[j], rows[:, 1]), "an output id is not an id of the segment"
    flat = i * k + j
    assert np.unique(flat).size == flat.size, "an (i, j) pair occurs twice"
    D, keep = np.zeros((k, k)), np.zeros((k, k), dtype=bool)
    D.ravel()[flat] = rows[:, 2]
    keep.ravel()[flat] = True
    return D, keep


def column_layout(ei, w=None):
    """A plain undirected edge list (both directions present) as a segment in the column layout: rows [row, col, w] sorted by
    (col, row), stable."""
    ei = np.asarray(ei, dtype=np.int64)
    w = np.ones(ei.shape[1]) if w is None else np.asarray(w, dtype=np.float64)
    o = np.lexsort((ei[0], ei[1]))
    return np.stack([ei[0][o].astype(np.float64), ei[1][o].astype(np.float64), w[o]], 1)


def symmetric_weights(ei, seed, lo=0.5, hi=2.0):
    """Random weights, uniform in [lo, hi], equal on (i, j) and (j, i)."""
    ei = np.asarray(ei, dtype=np.int64)
    rs = np.random.RandomState(seed)
    a, b = np.minimum(ei[0], ei[1]), np.maximum(ei[0], ei[1])
    n = int(ei.max()) + 1
    key = a * n + b
    uniq, inv = np.unique(key, return_inverse=True)
    return rs.uniform(lo, hi, uniq.size)[inv]
