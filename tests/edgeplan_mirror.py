"""Loader of the edge plan's host mirror (tests/csrc/edgeplan_mirror.cc around rlap_amd/csrc/rlap_edgeplan.h, rlap_gcnmath.h,
rlap_plan.h and rlap_spmm.h), shared by tests/test_edge_plan_cpu.py and the tests/test_gpu_edge_plan*.py files.  `plan` returns a
whole plan in the shape tests/plan_buffer.py decodes a device buffer into, so plan_buffer.same_decoded compares the two."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "csrc", "edgeplan_mirror.cc")
WEIGHTED, SELF_LOOPS, NORMALIZE, FORWARD, TRANSPOSED = 1, 2, 4, 256, 512
STATUS = {2: "an id is not an integer of its graph's range", 3: "a malformed table or a refused weight"}


class Refused(ValueError):
    def __init__(self, status):
        super().__init__(f"edge plan mirror: status {status} ({STATUS.get(status, '?')})")
        self.status = status


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libedgeplan_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    lib = ctypes.CDLL(so)
    i64, ci, vp, dbl = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    lib.edgeplan_lanes.restype = ci
    lib.edgeplan_accs.restype = ci
    lib.edgeplan_key_bits.restype = ctypes.c_uint
    lib.edgeplan_key_bits.argtypes = [i64]
    lib.edgeplan_places_consistent.restype = ci
    lib.edgeplan_places_consistent.argtypes = [i64]
    lib.edgeplan_build.restype = i64
    lib.edgeplan_build.argtypes = [i64, vp, i64, vp, i64, vp, i64, ci, dbl, ci] + [vp] * 11
    return lib


def flags_of(weighted=False, add_self_loops=True, normalize=True, directions="both"):
    return ((WEIGHTED if weighted else 0) | (SELF_LOOPS if add_self_loops else 0) | (NORMALIZE if normalize else 0)
            | {"forward": FORWARD, "transposed": TRANSPOSED, "both": FORWARD | TRANSPOSED}[directions])


def dir_cap(m, chunk=256):
    return 2 * m // chunk + 2 if m > chunk else 0


def plan(lib, rows, ptr, N, node_ptr=None, weighted=False, add_self_loops=True, fill_value=1.0, normalize=True, directions="both"):
    """The plan of (rows, ptr, N, node_ptr) by the mirror.  Raises Refused for an input the build refuses."""
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.float64).reshape(-1, 3))
    p = np.ascontiguousarray(np.asarray(ptr, dtype=np.int64))
    np_ = None if node_ptr is None else np.ascontiguousarray(np.asarray(node_ptr, dtype=np.int64))
    m, S, G = rows.shape[0], p.size - 1, 1 if np_ is None else np_.size - 1
    slots, cap = (S // G) * N, dir_cap(m)
    flags = flags_of(weighted, add_self_loops, normalize, directions)
    out = {"slots": slots, "loopc": None, "spans": [], "forward": None, "transposed": None}
    for t, name in enumerate(("forward", "transposed")):
        if not flags & (FORWARD, TRANSPOSED)[t]:
            continue
        deg, dis, lw, loopc = (np.full(slots, np.nan) for _ in range(4))
        off = np.full(slots + 1, -7, dtype=np.int64)
        rec_c, rec_id = np.full(m, np.nan), np.full(m, -7, dtype=np.int32)
        dslot, dk = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int64)
        chunks, removed = ctypes.c_int64(-1), ctypes.c_int64(-1)
        ent = lib.edgeplan_build(m, rows.ctypes.data, S, p.ctypes.data, G, None if np_ is None else np_.ctypes.data, N, flags & 7,
                                 float(fill_value), t, deg.ctypes.data, dis.ctypes.data, lw.ctypes.data, loopc.ctypes.data, off.ctypes.data,
                                 rec_c.ctypes.data, rec_id.ctypes.data, dslot.ctypes.data, dk.ctypes.data, ctypes.byref(chunks),
                                 ctypes.byref(removed))
        if ent < 0:
            raise Refused(-ent)
        out[name] = {"entries": int(ent), "chunks": int(chunks.value), "off": off, "c": rec_c[:ent].copy(), "id": rec_id[:ent].copy(),
                     "zero": np.zeros(ent, dtype=np.int32), "dir_slot": dslot[:chunks.value].copy(), "dir_k": dk[:chunks.value].copy()}
        out.update(deg=deg, dis=dis, lw=lw, loops_removed=int(removed.value))
        if flags & SELF_LOOPS:
            out["loopc"] = loopc
    return out


def entry_lists(dec, name, N):
    """Per layer (src, dst, val) of one direction of a decoded plan, the loops appended: what tests/spmm_mirror.entries takes.  For
    the transposed direction src / dst are swapped back, so the lists describe the same matrix."""
    d, slots = dec[name], dec["slots"]
    owner = np.repeat(np.arange(slots), np.diff(d["off"]))
    out = []
    for layer in range(slots // N if N else 0):
        sel = (owner >= layer * N) & (owner < (layer + 1) * N)
        own, other, val = owner[sel] - layer * N, d["id"][sel].astype(np.int64), d["c"][sel]
        if dec["loopc"] is not None:
            ar = np.arange(N)
            own, other, val = np.concatenate([own, ar]), np.concatenate([other, ar]), np.concatenate([val, dec["loopc"][layer * N:(layer + 1) * N]])
        out.append((own, other, val) if name == "transposed" else (other, own, val))
    return out
