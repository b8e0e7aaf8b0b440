"""Induced subgraphs and relabelling without a GPU: the rank arithmetic of rlap_amd/csrc/rlap_bitrank.h (compiled here with g++, the
same source rlap_subgraph.hip includes) against numpy cumsum, the host-side argument checks of ops.snapshot_subgraph, and the export."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_bitrank.h")

WRAP = r"""
#include <stddef.h>
#include <vector>
#include "rlap_bitrank.h"
extern "C" {
long long br_words_for(long long bits) { return rlap::bitrank::words_for(bits); }
int br_popc(unsigned long long w) { return rlap::bitrank::popc(w); }
// the kernels read (word, scan) side by side: build that table up to the word of x from the two arrays
static std::vector<rlap::bitrank::Rank> table(const unsigned long long* words, const long long* scan, long long x) {
    std::vector<rlap::bitrank::Rank> r((size_t)(x >> 6) + 1);
    for (size_t k = 0; k < r.size(); ++k) r[k] = rlap::bitrank::Rank{(uint64_t)words[k], scan ? (int64_t)scan[k] : 0};
    return r;
}
int br_test(const unsigned long long* words, long long x) { return rlap::bitrank::test(table(words, nullptr, x).data(), x) ? 1 : 0; }
long long br_before(const unsigned long long* words, const long long* scan, long long x) {
    return rlap::bitrank::before(table(words, scan, x).data(), x);
}
long long br_label(const unsigned long long* words, const long long* scan, long long lo, long long x) {
    return rlap::bitrank::label(table(words, scan, x).data(), lo, x);
}
int br_rank_bytes() { return (int)sizeof(rlap::bitrank::Rank); }
}
"""


@pytest.fixture(scope="module")
def br(tmp_path_factory):
    d = tmp_path_factory.mktemp("bitrank")
    src, so = d / "br.cc", d / "libbr.so"
    src.write_text(WRAP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.dirname(HDR),
                           "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    ll, up, lp = ctypes.c_longlong, ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_longlong)
    lib.br_words_for.restype = ll
    lib.br_words_for.argtypes = [ll]
    lib.br_popc.restype = ctypes.c_int
    lib.br_popc.argtypes = [ctypes.c_ulonglong]
    lib.br_test.restype = ctypes.c_int
    lib.br_test.argtypes = [up, ll]
    lib.br_before.restype = ll
    lib.br_before.argtypes = [up, lp, ll]
    lib.br_label.restype = ll
    lib.br_label.argtypes = [up, lp, ll, ll]
    assert lib.br_rank_bytes() == 16          # one 16-byte load per gather
    return lib


def pack(bits, br):
    """(words, scan) of a 0/1 vector the way the device lays them out: W words and a closing zero word, scan[k] = set bits in
    words[0 .. k) with scan[W] the total -- the scan itself from numpy (on the device it is a rocPRIM exclusive scan)."""
    nbits = len(bits)
    W = br.br_words_for(nbits)
    assert W == (nbits + 63) // 64
    padded = np.zeros((W + 1) * 64, dtype=np.uint64)
    padded[:nbits] = bits
    words = (padded.reshape(W + 1, 64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
    pc = np.array([br.br_popc(int(w)) for w in words], dtype=np.int64)
    assert np.array_equal(pc, padded.reshape(W + 1, 64).sum(1).astype(np.int64))
    scan = np.concatenate([[0], np.cumsum(pc)[:-1]]).astype(np.int64)
    return np.ascontiguousarray(words), np.ascontiguousarray(scan)


def ptrs(words, scan):
    return (words.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), scan.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))


@pytest.mark.parametrize("nbits", [1, 63, 64, 65, 127, 128, 129, 1000, 4096, 4100])
@pytest.mark.parametrize("density", [0.0, 0.03, 0.5, 1.0])
def test_before_equals_cumsum(br, nbits, density):
    rs = np.random.RandomState(nbits * 7 + int(density * 100))
    bits = (rs.rand(nbits) < density).astype(np.uint64)
    words, scan = pack(bits, br)
    wp, sp = ptrs(words, scan)
    ref = np.concatenate([[0], np.cumsum(bits.astype(np.int64))])     # ref[x] = set bits in front of x, x = nbits included
    for x in range(nbits + 1):
        assert br.br_before(wp, sp, x) == ref[x], x
    for x in range(nbits):
        assert br.br_test(wp, x) == int(bits[x])


@pytest.mark.parametrize("lo", [0, 1, 63, 64, 65, 127, 191])   # 63, 127, 191: the last bit of a word
def test_segment_labels_from_any_range_start(br, lo):
    """The label of id x inside a range that starts at bit lo (node_ptr[g], in general off the word grid) is its rank among the
    set bits of the range: numpy's searchsorted on the sorted ids of the range.  The range ends inside the last word."""
    nbits = 300                                          # 4 words and 44 bits
    rs = np.random.RandomState(lo)
    bits = (rs.rand(nbits) < 0.4).astype(np.uint64)
    bits[lo] = 1                                         # the first id of the range is in the set ...
    words, scan = pack(bits, br)
    wp, sp = ptrs(words, scan)
    for hi in (lo + 1, lo + 2, 256, 257, nbits):         # ... and ranges of one id, up to the word edge, and to the last bit
        ids = lo + np.nonzero(bits[lo:hi])[0]
        for x in ids:
            assert br.br_label(wp, sp, lo, int(x)) == np.searchsorted(ids, x)
        assert br.br_label(wp, sp, lo, hi) == len(ids)   # the count of the range: ids_ptr[s + 1] - ids_ptr[s]
    bits[lo] = 0                                         # ... or not
    words, scan = pack(bits, br)
    wp, sp = ptrs(words, scan)
    ids = lo + np.nonzero(bits[lo:])[0]
    for x in ids:
        assert br.br_label(wp, sp, lo, int(x)) == np.searchsorted(ids, x)


def test_empty_ranges_and_empty_bitmap(br):
    bits = np.zeros(130, dtype=np.uint64)
    bits[[0, 64, 129]] = 1
    words, scan = pack(bits, br)
    wp, sp = ptrs(words, scan)
    for lo in (0, 1, 63, 64, 65, 129, 130):
        assert br.br_label(wp, sp, lo, lo) == 0          # an empty range [lo, lo)
    assert br.br_label(wp, sp, 1, 64) == 0 and br.br_label(wp, sp, 65, 129) == 0   # ranges without a set bit
    assert br.br_before(wp, sp, 130) == 3
    words, scan = pack(np.zeros(0, dtype=np.uint64), br)  # no bits at all: the closing word alone
    wp, sp = ptrs(words, scan)
    assert len(words) == 1 and br.br_before(wp, sp, 0) == 0


# ---------------------------------------------------------------- host-side argument checks (nothing is launched: no GPU here)
SC = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], dtype=torch.float64)


@pytest.mark.parametrize("args,kw", [
    ((SC, [0, 2], 2), {"nodes_ptr": [0, 1]}),                                     # nodes_ptr without nodes
    ((SC, [0, 2], 2), {"nodes": torch.tensor([0, 1]), "nodes_ptr": [0, 1, 2]}),    # wrong length: 2 segments' worth for 1
    ((SC, [0, 1, 2], 2), {"nodes": torch.tensor([0, 1]), "nodes_ptr": [0, 2]}),    # wrong length: 1 for 2
    ((SC, [0, 1, 2], 2), {"nodes": torch.tensor([0, 1]), "nodes_ptr": [0, 2, 1]}),  # decreasing
    ((SC, [0, 1, 2], 2), {"nodes": torch.tensor([0, 1]), "nodes_ptr": [0, 1, 1]}),  # does not end at len(nodes)
    ((SC, [0, 1, 2], 2), {"nodes": torch.tensor([0, 1]), "nodes_ptr": [1, 1, 2]}),  # does not start at 0
    ((SC, [0, 2], 2), {"nodes": torch.tensor([0.0, 1.0])}),                        # non-integer nodes
    ((SC, [0, 2], 2), {"nodes": torch.tensor([True, False])}),
    ((SC, [0, 2], 2), {"nodes": [0.5, 1]}),
    ((SC, [0, 2], 2), {"nodes": torch.tensor([[0, 1]])}),                          # not 1-D
    ((SC, [0, 3], 2), {}),                               # ptr[-1] != rows
    ((SC, [1, 2], 2), {}),                               # ptr[0] != 0
    ((SC, [0, 2, 1, 2], 2), {}),                         # decreasing
    ((SC, [0], 2), {}),                                  # no segment, but rows
    ((SC[:0], [1], 2), {}),                              # no segment: ptr must be [0]
    ((SC, [0, 2], -1), {}),                              # num_nodes
    ((SC[:, :2], [0, 2], 2), {}),                        # not (m, 3)
    ((SC, [0, 1, 2], 2), {"node_ptr": [0, 1, 2, 2]}),   # 3 graphs do not divide 2 segments
    ((SC, [0, 2], 2), {"node_ptr": [0, 1]}),            # node_ptr[-1] != num_nodes
    ((SC[:0], [0], 2), {"node_ptr": [0, 1]}),           # the same without a segment
])
def test_snapshot_subgraph_bad_arguments(args, kw):
    from rlap_amd import ops
    with pytest.raises(ValueError):
        ops.snapshot_subgraph(*args, **kw)


def test_argument_errors_are_those_of_snapshot_ppr():
    """ptr / node_ptr mistakes are refused with the very messages snapshot_ppr gives (one checker for all snapshot calls)."""
    from rlap_amd import ops
    for args, kw in [((SC, [0, 3], 2), {}), ((SC, [0, 2, 1, 2], 2), {}), ((SC, [0, 1, 2], 2), {"node_ptr": [0, 1, 2, 2]}),
                     ((SC, [0, 2], 2), {"node_ptr": [0, 1]})]:
        with pytest.raises(ValueError) as e1:
            ops.snapshot_ppr(*args, **kw)
        with pytest.raises(ValueError) as e2:
            ops.snapshot_subgraph(*args, **kw)
        assert str(e1.value) == str(e2.value)


def test_valid_arguments_reach_the_device_check():
    """Well-formed arguments pass every host-side check: what stops the call on a box without a GPU is the missing device
    (RuntimeError), not a ValueError."""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from rlap_amd import ops
    for kw in [{}, {"nodes": [1, 0, 1]}, {"nodes": torch.tensor([1, 0]), "nodes_ptr": [0, 2]}, {"node_ptr": [0, 2], "relabel": True},
               {"nodes": [], "nodes_ptr": [0, 0], "remove_self_loops": True}]:
        with pytest.raises(RuntimeError):
            ops.snapshot_subgraph(SC, [0, 2], 2, **kw)
    with pytest.raises(RuntimeError):
        ops.snapshot_subgraph(SC[:0], [0], 2)


def test_export_and_flags():
    from rlap_amd import _lib
    assert "rlap_snapshot_subgraph" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "rlap_snapshot_subgraph")
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert f"RLAP_SUB_RELABEL = {_lib.SUB_RELABEL}" in hdr and f"RLAP_SUB_NO_SELF_LOOPS = {_lib.SUB_NO_SELF_LOOPS}" in hdr
    # a NULL handle is refused before anything else is looked at
    assert lib.rlap_snapshot_subgraph(None, None, 0, None, 0, None, 1, 0, None, None, 0, 0, None, None, None, 0, None, None) == 3

