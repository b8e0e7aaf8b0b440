"""Propagation plans without a GPU: the layout rules of rlap_amd/csrc/rlap_plan.h (a slot's offset, an entry's place with and
without dropped loop rows, the chunk directory), compiled here with g++ through tests/csrc/plan_mirror.cc -- the same functions
rlap_plan.hip's kernels read.  The lists they give for a small hand-made input and for a star with 600 leaves are checked against
a straightforward Python construction, and rlap_spmm.h's rule over them against tests/csrc/spmm_mirror.cc bit for bit, forward and
transposed.  The same file, built as a stand-alone program under -fsanitize=address,undefined, runs once on those inputs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import plan_buffer
import spmm_mirror

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "plan_mirror.cc")
INC = os.path.join(ROOT, "rlap_amd", "csrc")


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan")
    so = os.path.join(str(d), "libplan_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC, "-o", so, SRC])
    lib = ctypes.CDLL(so)
    i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    for name in ("plan_record_bytes", "plan_chunkref_bytes"):
        getattr(lib, name).restype = i64
        getattr(lib, name).argtypes = []
    lib.plan_dir_cap.restype = i64
    lib.plan_dir_cap.argtypes = [i64]
    lib.plan_layout.restype = None
    lib.plan_layout.argtypes = [i64, i64, ci, ci, ci, vp]
    lib.plan_build.restype = i64
    lib.plan_build.argtypes = [i64, vp, i64, vp, i64, i64, vp, ci, ci, vp, vp, vp, vp, vp, vp]
    lib.plan_dir_first.restype = i64
    lib.plan_dir_first.argtypes = [i64, vp, i64]
    lib.plan_product.restype = ci
    lib.plan_product.argtypes = [i64, i64, i64, vp, vp, vp, i64, vp, vp, vp, ci, vp, vp]
    return lib, spmm_mirror.build(d)


HAND = [[1, 0, 0.5], [0, 0, 3.0], [2, 0, 0.25], [0, 0, 4.0],     # two loop rows of id 0
        [0, 1, 0.5],
        [0, 2, 0.25], [2, 2, 7.0],
        [5, 5, 2.0]]                                              # an id with nothing but a loop row


def hand_input():
    rows = np.array(HAND + HAND, dtype=np.float64)
    return rows, [0, 8, 16], 7


def star_input(leaves=600):
    """The centre's block (one row per leaf, two loop rows inside it), then one block per leaf."""
    centre = [[i + 1, 0, 0.5 + 0.001 * i] for i in range(leaves)]
    centre.insert(300, [0, 0, 1.5])
    centre.insert(3, [0, 0, 2.5])
    rows = centre + [[0, i + 1, 0.5 + 0.001 * i] for i in range(leaves)]
    return np.array(rows, dtype=np.float64), [0, len(rows)], leaves + 1


def build(lib, rows, ptr, N, c, drop, transpose):
    m, S = rows.shape[0], len(ptr) - 1
    slots, cap = S * N, lib.plan_dir_cap(m)
    p = np.array(ptr, dtype=np.int64)
    off = np.full(slots + 1, -7, dtype=np.int64)
    rec_c, rec_id = np.full(m, np.nan), np.full(m, -7, dtype=np.int32)
    dslot, dk = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int64)
    chunks = ctypes.c_int64(-1)
    rows = np.ascontiguousarray(rows)
    ent = lib.plan_build(m, rows.ctypes.data, S, p.ctypes.data, 1, N, c.ctypes.data, int(drop), int(transpose), off.ctypes.data,
                         rec_c.ctypes.data, rec_id.ctypes.data, dslot.ctypes.data, dk.ctypes.data, ctypes.byref(chunks))
    return ent, off, rec_c, rec_id, dslot, dk, chunks.value


def python_lists(rows, ptr, N, c, drop, transpose):
    """{slot: [(coefficient, id taken)]}: every list by appending in input order (tests/plan_buffer.py, one graph a layer)."""
    return {slot: [(c[r], i) for r, i in l] for slot, l in plan_buffer.expected_lists(rows, ptr, N, 1, drop, transpose).items()}


@pytest.mark.parametrize("which", ["hand", "star"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("transpose", [False, True])
def test_lists_against_a_python_construction_and_the_summation_mirror(libs, which, drop, transpose):
    lib, spmm = libs
    C = spmm.spmm_chunk()
    rows, ptr, N = hand_input() if which == "hand" else star_input()
    m, S = rows.shape[0], len(ptr) - 1
    rs = np.random.RandomState(7)
    c = rs.rand(m) + 0.25
    ent, off, rec_c, rec_id, dslot, dk, chunks = build(lib, rows, ptr, N, c, drop, transpose)
    lists = python_lists(rows, ptr, N, c, drop, transpose)
    # a slot's offset, an entry's place
    assert ent == sum(len(l) for l in lists.values()) == off[-1] and off[0] == 0
    assert ent == (m - int((rows[:, 0] == rows[:, 1]).sum()) if drop else m)
    for slot in range(S * N):
        want = lists.get(slot, [])
        got = list(zip(rec_c[off[slot]:off[slot + 1]].tolist(), rec_id[off[slot]:off[slot + 1]].tolist()))
        assert got == want, (slot, got[:4], want[:4])
    # the chunk directory: the lists longer than C, in slot order, every chunk with its slot and its number
    want_dir = [(slot, k) for slot in sorted(lists) if len(lists[slot]) > C for k in range(-(-len(lists[slot]) // C))]
    assert chunks == len(want_dir) and list(zip(dslot[:chunks].tolist(), dk[:chunks].tolist())) == want_dir
    assert chunks <= lib.plan_dir_cap(m)
    if which == "star":
        assert chunks == 3 and want_dir[0][0] == 0                           # 600 entries of the centre: three chunks
        assert lib.plan_dir_first(chunks, dslot.ctypes.data, 0) == 0 and lib.plan_dir_first(chunks, dslot.ctypes.data, 1) == 3
    else:
        assert chunks == 0
    # the sum over the plan's lists is spmm_mirror's over the entry list, bit for bit
    F = 3
    x = rs.randn(N, F) * 10.0 ** rs.randint(-2, 3, (N, F))
    loopc = rs.rand(S * N) + 0.5
    y = np.full((S * N, F), np.nan)
    rc = lib.plan_product(S * N, N, F, off.ctypes.data, rec_c.ctypes.data, rec_id.ctypes.data, chunks, dslot.ctypes.data, dk.ctypes.data,
                          x.ctypes.data, int(drop), loopc.ctypes.data, y.ctypes.data)
    assert rc == 0, "the directory does not lead to the chunks of a long list, or their sum differs from the list's"
    for s in range(S):
        part = rows[ptr[s]:ptr[s + 1]]
        src, dst, val = part[:, 0].astype(np.int64), part[:, 1].astype(np.int64), c[ptr[s]:ptr[s + 1]]
        if drop:   # the list rlap_snapshot_gcn_norm would give: the rows that stay, then one loop per id
            keep = src != dst
            ar = np.arange(N)
            src, dst, val = np.concatenate([src[keep], ar]), np.concatenate([dst[keep], ar]), np.concatenate([val[keep], loopc[s * N:(s + 1) * N]])
        ref = spmm_mirror.entries(spmm, src, dst, val, N, x, drop, transpose)
        assert np.array_equal(y[s * N:(s + 1) * N].view(np.int64), ref.view(np.int64)), (which, drop, transpose, s)


def test_layout_of_the_buffer(libs):
    lib, _ = libs
    assert lib.plan_record_bytes() == 16 and lib.plan_chunkref_bytes() == 16
    assert lib.plan_dir_cap(256) == 0 and lib.plan_dir_cap(257) == 4 and lib.plan_dir_cap(5120) == 42

    def layout(m, slots, loops, fwd, tr):
        out = np.zeros(8, dtype=np.int64)
        lib.plan_layout(m, slots, int(loops), int(fwd), int(tr), out.ctypes.data)
        return dict(zip(("loop", "off_f", "off_t", "dir_f", "dir_t", "rec_f", "rec_t", "bytes"), out.tolist()))

    L = layout(1000, 70, True, True, True)
    parts = [("loop", 8 * 70), ("off_f", 8 * 71), ("off_t", 8 * 71), ("dir_f", 16 * lib.plan_dir_cap(1000)), ("dir_t", 16 * lib.plan_dir_cap(1000)),
             ("rec_f", 16000), ("rec_t", 16000)]
    at = 0
    for name, size in parts:                                                  # in this order, 256-byte aligned, none overlapping
        assert L[name] == at and at % 256 == 0, name
        at = (at + size + 255) // 256 * 256
    assert L["bytes"] == at
    one = layout(1000, 70, False, True, False)
    assert one["loop"] == -1 and one["off_t"] == one["dir_t"] == one["rec_t"] == -1 and one["off_f"] == 0 and one["bytes"] < L["bytes"]
    assert layout(0, 0, True, True, True)["bytes"] >= 256


def test_the_mirror_under_asan_and_ubsan(tmp_path):
    """The same file as a stand-alone program with its own main: a plain executable, nothing preloaded."""
    exe = tmp_path / "plan_mirror_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-DPLAN_MIRROR_MAIN", "-I", INC, "-o", str(exe), SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": ok (0)") == 8 and "FAILED" not in r.stdout
