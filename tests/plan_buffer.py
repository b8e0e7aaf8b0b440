"""A decoder of the plan buffer's public format and an independent construction of what it must hold, shared by
tests/test_plan_buffer_cpu.py, tests/test_gpu_plan_buffer.py, tests/test_gpu_plan_cabi.py and tests/test_plan_cpu.py.

The format is the one include/rlap_hip.h documents for rlap_snapshot_plan_build: with slots = (segments / graphs) * num_nodes,
    loopc  double[slots]                         at desc.loop_offset, with RLAP_GCN_SELF_LOOPS
and per direction that was built (RLAP_PLAN_FORWARD / RLAP_PLAN_TRANSPOSED in desc.flags)
    off    int64[slots + 1]                      at desc.off_*
    dir    {int64 slot, int64 k}[desc.chunks_*]  at desc.dir_*
    rec    {double c, int32 id, int32 0}[desc.entries_*]  at desc.rec_*
Nothing here includes a header of the library or calls it: the sizes are written out."""
import numpy as np

GCN_SELF_LOOPS, PLAN_FORWARD, PLAN_TRANSPOSED = 2, 256, 512
RECORD = np.dtype([("c", "<f8"), ("id", "<i4"), ("zero", "<i4")])
CHUNKREF = np.dtype([("slot", "<i8"), ("k", "<i8")])
assert RECORD.itemsize == 16 and CHUNKREF.itemsize == 16
DIRECTIONS = (("forward", PLAN_FORWARD), ("transposed", PLAN_TRANSPOSED))


def _part(raw, spans, name, offset, dtype, count):
    offset, count = int(offset), int(count)
    end = offset + count * np.dtype(dtype).itemsize
    if offset < 0 or count < 0 or end > raw.size:
        raise ValueError(f"{name}: bytes [{offset}, {end}) are not inside the {raw.size} bytes given")
    spans.append((name, offset, end))
    return np.frombuffer(raw, dtype=dtype, count=count, offset=offset).copy()


def decode(raw, desc):
    """The content of a plan buffer by the descriptor's offsets alone.  `raw`: bytes or a uint8 array; `desc`: anything with the
    fields of rlap_plan_desc.  Returns {"slots", "loopc" (or None), "forward" / "transposed" (None when not built), "spans"};
    a direction is {"entries", "chunks", "off", "c", "id", "zero", "dir_slot", "dir_k"}, `spans` the (name, begin, end) byte ranges
    that were read.  Padding, records past `entries` and directory entries past `chunks` are never looked at."""
    if isinstance(raw, np.ndarray):
        assert raw.dtype == np.uint8, raw.dtype
        raw = np.ascontiguousarray(raw).reshape(-1)
    else:
        raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    slots = (int(desc.segments) // int(desc.graphs)) * int(desc.num_nodes)
    flags = int(desc.flags)
    spans = []
    out = {"slots": slots, "loopc": None, "spans": spans}
    if flags & GCN_SELF_LOOPS:
        out["loopc"] = _part(raw, spans, "loopc", desc.loop_offset, "<f8", slots)
    for name, bit in DIRECTIONS:
        if not flags & bit:
            out[name] = None
            continue
        entries, chunks = int(getattr(desc, "entries_" + name)), int(getattr(desc, "chunks_" + name))
        off = _part(raw, spans, "off_" + name, getattr(desc, "off_" + name), "<i8", slots + 1)
        rec = _part(raw, spans, "rec_" + name, getattr(desc, "rec_" + name), RECORD, entries)
        ref = _part(raw, spans, "dir_" + name, getattr(desc, "dir_" + name), CHUNKREF, chunks)
        out[name] = {"entries": entries, "chunks": chunks, "off": off,
                     "c": np.ascontiguousarray(rec["c"]), "id": np.ascontiguousarray(rec["id"]), "zero": np.ascontiguousarray(rec["zero"]),
                     "dir_slot": np.ascontiguousarray(ref["slot"]), "dir_k": np.ascontiguousarray(ref["k"])}
    return out


def same_decoded(a, b):
    """Whether two decoded buffers hold the same bits (the coefficients compared as integers)."""
    if a["slots"] != b["slots"] or (a["loopc"] is None) != (b["loopc"] is None):
        return False
    if a["loopc"] is not None and not np.array_equal(a["loopc"].view(np.int64), b["loopc"].view(np.int64)):
        return False
    for name, _ in DIRECTIONS:
        da, db = a[name], b[name]
        if (da is None) != (db is None):
            return False
        if da is None:
            continue
        if (da["entries"], da["chunks"]) != (db["entries"], db["chunks"]):
            return False
        for key in ("off", "id", "zero", "dir_slot", "dir_k"):
            if not np.array_equal(da[key], db[key]):
                return False
        if not np.array_equal(da["c"].view(np.int64), db["c"].view(np.int64)):
            return False
    return True


def expected_lists(rows, ptr, N, G, drop_loops, transpose):
    """{slot: [(row index, id taken)]}: every list by appending in input order.  rows (m, 3) [row, col, w]; the segments of `ptr`
    are layers of G graphs each (layer = segment // G); slot = layer * N + the target (transposed: the source) of the row;
    drop_loops: the rows with row == col leave the lists."""
    rows = np.asarray(rows)
    ptr = [int(v) for v in ptr]
    lists = {}
    for s in range(len(ptr) - 1):
        layer = s // G
        for r in range(ptr[s], ptr[s + 1]):
            vi, vj = int(rows[r, 0]), int(rows[r, 1])
            if drop_loops and vi == vj:
                continue
            lists.setdefault(layer * N + (vi if transpose else vj), []).append((r, vj if transpose else vi))
    return lists


def expected_directory(lists, chunk):
    """[(slot, k)]: the lists longer than `chunk`, in slot order, every chunk once."""
    return [(slot, k) for slot in sorted(lists) if len(lists[slot]) > chunk for k in range(-(-len(lists[slot]) // chunk))]


def entry_numbers(rows, ptr, N, G, node_ptr, loops):
    """Where the entry list of rlap_snapshot_gcn_norm holds every row and every loop, by the order it documents: per segment, the
    rows that stay in input order, then (loops) one loop per id of the segment's graph.  Returns (row_at[m] with -1 for a dropped
    loop row, loop_at[(S / G) N] or None, eptr[S + 1])."""
    rows = np.asarray(rows)
    ptr = [int(v) for v in ptr]
    S = len(ptr) - 1
    row_at = np.full(rows.shape[0], -1, dtype=np.int64)
    loop_at = np.full((S // G) * N, -1, dtype=np.int64) if loops else None
    eptr, at = [0], 0
    for s in range(S):
        lo, hi = (int(node_ptr[s % G]), int(node_ptr[s % G + 1])) if node_ptr is not None else (0, N)
        for r in range(ptr[s], ptr[s + 1]):
            if loops and rows[r, 0] == rows[r, 1]:
                continue
            row_at[r] = at
            at += 1
        if loops:
            loop_at[(s // G) * N + lo:(s // G) * N + hi] = np.arange(at, at + hi - lo)
            at += hi - lo
        eptr.append(at)
    return row_at, loop_at, eptr
