"""tests/plan_buffer.py's decoder against the layout header, without a GPU: the arrays that tests/csrc/plan_mirror.cc's plan_build
returns (the layout rules of rlap_amd/csrc/rlap_plan.h) are packed into one byte buffer at the offsets plan_layout returns, every
gap filled with 0xA5, and decoded with a descriptor made of the same numbers.  Every array comes back exactly, so the decoder reads
the documented format before it ever meets a device buffer."""
from types import SimpleNamespace

import numpy as np
import pytest

import plan_buffer
from test_plan_cpu import build, hand_input, libs, star_input  # noqa: F401  (libs is a fixture)

FILL = 0xA5


def pack(lib, rows, ptr, N, drop, directions, seed):
    """(buffer, descriptor, what went in) for one input; drop: loop rows leave the lists and the plan has loop coefficients."""
    m, S = rows.shape[0], len(ptr) - 1
    slots = S * N
    rs = np.random.RandomState(seed)
    c = rs.rand(m) + 0.25
    want = {"forward": directions in ("both", "forward"), "transposed": directions in ("both", "transposed")}
    L = np.zeros(8, dtype=np.int64)
    lib.plan_layout(m, slots, int(drop), int(want["forward"]), int(want["transposed"]), L.ctypes.data)
    L = dict(zip(("loop", "off_forward", "off_transposed", "dir_forward", "dir_transposed", "rec_forward", "rec_transposed", "bytes"), L.tolist()))
    buf = np.full(L["bytes"], FILL, dtype=np.uint8)

    def put(offset, array):
        b = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert offset >= 0 and offset % 256 == 0 and offset + b.size <= buf.size
        assert bool((buf[offset:offset + b.size] == FILL).all()), "two parts overlap"
        buf[offset:offset + b.size] = b

    src = {"loopc": None}
    flags = (plan_buffer.GCN_SELF_LOOPS if drop else 0)
    if drop:
        src["loopc"] = rs.rand(slots) + 0.5
        put(L["loop"], src["loopc"])
    else:
        assert L["loop"] == -1
    desc = SimpleNamespace(m=m, segments=S, graphs=1, num_nodes=N, fill_value=1.0, loop_offset=L["loop"], plan_bytes=L["bytes"], magic=0x504C414E)
    for t, (name, bit) in enumerate(plan_buffer.DIRECTIONS):
        for part in ("off_", "dir_", "rec_"):
            setattr(desc, part + name, L[part + name])
        if not want[name]:
            assert L["off_" + name] == L["dir_" + name] == L["rec_" + name] == -1
            setattr(desc, "entries_" + name, -1)
            setattr(desc, "chunks_" + name, -1)
            src[name] = None
            continue
        flags |= bit
        ent, off, rec_c, rec_id, dslot, dk, chunks = build(lib, rows, ptr, N, c, drop, bool(t))
        assert ent >= 0 and chunks <= dslot.size
        put(L["off_" + name], off)
        ref = np.zeros(dslot.size, dtype=plan_buffer.CHUNKREF)       # (past `chunks` the mirror's filler: unspecified content)
        ref["slot"], ref["k"] = dslot, dk
        put(L["dir_" + name], ref)
        rec = np.zeros(ent, dtype=plan_buffer.RECORD)                # (past `entries` the gap's filler stays)
        rec["c"], rec["id"] = rec_c[:ent], rec_id[:ent]
        put(L["rec_" + name], rec)
        setattr(desc, "entries_" + name, ent)
        setattr(desc, "chunks_" + name, chunks)
        src[name] = (ent, off, rec_c[:ent], rec_id[:ent], dslot[:chunks], dk[:chunks], chunks)
    desc.flags = flags
    return buf, desc, src


@pytest.mark.parametrize("directions", ["both", "forward", "transposed"])
@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("which", ["hand", "star"])
def test_decode_returns_what_was_packed(libs, which, drop, directions):
    lib, _ = libs
    rows, ptr, N = hand_input() if which == "hand" else star_input()
    buf, desc, src = pack(lib, rows, ptr, N, drop, directions, seed=3)
    for raw in (buf, buf.tobytes()):
        got = plan_buffer.decode(raw, desc)
        assert got["slots"] == (len(ptr) - 1) * N
        if drop:
            assert np.array_equal(got["loopc"].view(np.int64), src["loopc"].view(np.int64))
        else:
            assert got["loopc"] is None
        for name, _ in plan_buffer.DIRECTIONS:
            if src[name] is None:
                assert got[name] is None
                continue
            ent, off, rec_c, rec_id, dslot, dk, chunks = src[name]
            d = got[name]
            assert (d["entries"], d["chunks"]) == (ent, chunks)
            assert d["off"].dtype == np.int64 and np.array_equal(d["off"], off) and d["off"][-1] == ent
            assert d["c"].dtype == np.float64 and d["c"].shape == (ent,) and np.array_equal(d["c"].view(np.int64), rec_c.view(np.int64))
            assert d["id"].dtype == np.int32 and np.array_equal(d["id"], rec_id)
            assert d["zero"].dtype == np.int32 and d["zero"].shape == (ent,) and not d["zero"].any()
            assert np.array_equal(d["dir_slot"], dslot) and np.array_equal(d["dir_k"], dk)
            if which == "star":
                assert chunks == 3
        for _, lo, hi in got["spans"]:                                          # nothing decoded is a byte of a gap
            assert 0 <= lo <= hi <= desc.plan_bytes
        assert plan_buffer.same_decoded(got, plan_buffer.decode(buf, desc))
    # the lists the decoded arrays hold are the plain construction's
    for t, (name, _) in enumerate(plan_buffer.DIRECTIONS):
        if src[name] is None:
            continue
        d = plan_buffer.decode(buf, desc)[name]
        lists = plan_buffer.expected_lists(rows, ptr, N, 1, drop, bool(t))
        for slot in range(got["slots"]):
            assert d["id"][d["off"][slot]:d["off"][slot + 1]].tolist() == [i for _, i in lists.get(slot, [])], (name, slot)
        C = libs[1].spmm_chunk()
        assert list(zip(d["dir_slot"].tolist(), d["dir_k"].tolist())) == plan_buffer.expected_directory(lists, C)


def test_decode_notices_a_changed_byte_and_refuses_a_short_buffer(libs):
    lib, _ = libs
    rows, ptr, N = star_input()
    buf, desc, _ = pack(lib, rows, ptr, N, True, "both", seed=4)
    ref = plan_buffer.decode(buf, desc)
    for where in (desc.rec_forward + 12, desc.rec_transposed + 16 * (desc.entries_transposed - 1) + 8, desc.dir_forward + 8,
                  desc.off_transposed + 8 * ref["slots"], desc.loop_offset):
        bad = buf.copy()
        bad[where] ^= 1
        assert not plan_buffer.same_decoded(ref, plan_buffer.decode(bad, desc)), where
    gap = buf.copy()                                                            # a record past `entries` is not looked at
    gap[desc.rec_forward + 16 * desc.entries_forward:desc.rec_transposed] = 0
    assert plan_buffer.same_decoded(ref, plan_buffer.decode(gap, desc))
    with pytest.raises(ValueError, match="rec_transposed"):
        plan_buffer.decode(buf[:desc.rec_transposed + 16 * desc.entries_transposed - 1], desc)


def test_entry_numbers_follow_the_documented_order():
    rows, ptr, N = hand_input()
    row_at, loop_at, eptr = plan_buffer.entry_numbers(rows, ptr, N, 1, None, True)
    assert eptr == [0, 4 + 7, 2 * (4 + 7)]
    assert row_at.tolist() == [0, -1, 1, -1, 2, 3, -1, -1, 11, -1, 12, -1, 13, 14, -1, -1]
    assert loop_at.tolist() == list(range(4, 11)) + list(range(15, 22))
    row_at, loop_at, eptr = plan_buffer.entry_numbers(rows, ptr, N, 1, None, False)
    assert loop_at is None and row_at.tolist() == list(range(16)) and eptr == [0, 8, 16]
    # two graphs a layer: the loops of a segment are its graph's ids
    row_at, loop_at, eptr = plan_buffer.entry_numbers(rows, [0, 8, 8, 16, 16], N, 2, [0, 3, 7], True)
    assert eptr == [0, 4 + 3, 4 + 3 + 4, 4 + 3 + 4 + 4 + 3, 4 + 3 + 4 + 4 + 3 + 4]
    assert loop_at.tolist() == [4, 5, 6, 7, 8, 9, 10, 15, 16, 17, 18, 19, 20, 21]
