"""The C ABI of the propagation plans without a GPU: rlap_snapshot_plan_bytes is host arithmetic and answers on the real library;
the two new structures of include/rlap_hip.h and their ctypes twins in rlap_amd._lib describe the same bytes."""
import ctypes
import os
import re

import pytest

from rlap_amd import _lib
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, TOO_LARGE = 0, 3, 9
LIST = _lib.GCN_WEIGHTED | _lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE
FWD, TR = _lib.PLAN_FORWARD, _lib.PLAN_TRANSPOSED


def query(m, S, G, n, flags):
    b = ctypes.c_size_t(0)
    rc = _lib.load().rlap_snapshot_plan_bytes(m, S, G, n, flags, ctypes.byref(b))
    return rc, b.value


def size(m, S, G, n, flags):
    rc, b = query(m, S, G, n, flags)
    assert rc == OK, (m, S, G, n, flags, rc)
    return b


def test_size_query_refuses_what_a_build_would():
    assert query(-1, 6, 1, 100, LIST)[0] == BAD_ARG
    assert query(10, 6, 1, -1, LIST)[0] == BAD_ARG
    assert query(10, 0, 1, 100, LIST)[0] == BAD_ARG and query(10, 6, 0, 100, LIST)[0] == BAD_ARG
    assert query(10, 6, 4, 100, LIST)[0] == BAD_ARG                          # graphs that do not divide the segments
    for flag in (_lib.GCN_F32, _lib.SPMM_TRANSPOSE, _lib.SPMM_X_F32, _lib.SPMM_X_PER_LAYER, 128, 1024):   # not this call's
        assert query(10, 6, 1, 100, LIST | flag)[0] == BAD_ARG, flag
    assert query(1 << 31, 6, 1, 100, LIST)[0] == TOO_LARGE                   # the int32 row numbering
    assert query((1 << 31) - 1, 6, 1, 100, LIST)[0] == TOO_LARGE
    assert query(10, 1 << 30, 1, 100, LIST)[0] == TOO_LARGE
    assert query(10, 6, 1, (1 << 31) - 1, LIST)[0] == TOO_LARGE
    assert query(10, 1 << 20, 1, 1 << 20, LIST)[0] == TOO_LARGE              # 2^40 (layer, id) slots
    assert _lib.load().rlap_snapshot_plan_bytes(10, 6, 1, 100, LIST, None) == BAD_ARG


def test_size_query_is_a_bound_that_grows_with_the_input():
    ms = [0, 1, 255, 256, 257, 1000, 4096, 10 ** 6, 10 ** 8]
    ns = [0, 1, 7, 1000, 10 ** 6]
    for flags in (LIST, LIST | FWD, LIST | TR, LIST | FWD | TR, 0, FWD):
        for n in ns:
            sizes = [size(m, 6, 1, n, flags) for m in ms]
            assert sizes == sorted(sizes), (flags, n)                        # monotone in m
        for m in ms:
            sizes = [size(m, 6, 1, n, flags) for n in ns]
            assert sizes == sorted(sizes), (flags, m)                        # and in num_nodes
    for m in ms:
        for n in ns:
            both, fwd, tr = size(m, 6, 1, n, LIST), size(m, 6, 1, n, LIST | FWD), size(m, 6, 1, n, LIST | TR)
            assert both == size(m, 6, 1, n, LIST | FWD | TR)                 # neither bit: both directions
            assert both >= fwd and both >= tr and fwd > 0 and tr > 0
            assert fwd >= 12 * m + 8 * 6 * n and tr >= 12 * m + 8 * 6 * n    # at least 12 bytes per row and direction, and the offsets
            assert both >= 2 * 12 * m
            assert size(m, 6, 1, n, LIST) >= size(m, 6, 1, n, 0)             # the loop coefficients
    assert size(1000, 6, 2, 50, LIST) == size(1000, 3, 1, 50, LIST)          # three layers either way


@pytest.mark.parametrize("c_name,py_name", [("rlap_plan_desc", "PlanDesc"), ("rlap_plan_info", "PlanInfo")])
def test_plan_structs_match_the_header(tmp_path, c_name, py_name):
    layout_matches_the_header(tmp_path, c_name, py_name)


def test_exports_and_flags_are_declared():
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    for name in ("rlap_snapshot_plan_bytes", "rlap_snapshot_plan_build", "rlap_snapshot_plan_propagate"):
        assert name in _lib.EXPORTS and re.search(r"\bint %s\(" % name, hdr)
    m = re.search(r"enum \{ RLAP_PLAN_FORWARD = (\d+), RLAP_PLAN_TRANSPOSED = (\d+) \}", hdr)
    assert tuple(int(v) for v in m.groups()) == (_lib.PLAN_FORWARD, _lib.PLAN_TRANSPOSED)
    used = [_lib.GCN_WEIGHTED, _lib.GCN_SELF_LOOPS, _lib.GCN_NORMALIZE, _lib.GCN_F32, _lib.SPMM_TRANSPOSE, _lib.SPMM_X_F32, _lib.SPMM_X_PER_LAYER]
    assert all(_lib.PLAN_FORWARD & f == 0 and _lib.PLAN_TRANSPOSED & f == 0 for f in used)   # no bit shared with the other calls' flags
    plan_h = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_plan.h")).read()
    assert int(re.search(r"MAGIC\s*=\s*(0x[0-9a-fA-F]+)", plan_h).group(1), 16) == _lib.PLAN_MAGIC
