"""Edge adding without a GPU (rlap_edge_add, ops.add_edges).

1. The rules of rlap_amd/csrc/rlap_edgeadd.h -- compiled here with g++ through tests/csrc/edgeadd_mirror.cc, the same functions
   rlap_edgeadd.hip's kernels read -- against restatements written from the prose of the contract alone: the coin and the pick in
   pure-Python integers and fractions, the structure of a view in numpy (np.unique, np.add.at) and, for general weights, a Python
   loop that adds in input order.  Everything is compared by equality.
2. The mirror as a stand-alone program under -fsanitize=address,undefined, malformed inputs included.
3. The Python -> C mapping of ops.add_edges and the adapters on a stub library, every ValueError raised before a call is made, the
   layout of rlap_edge_add_info, and the export's place in the header, _lib.EXPORTS, the Makefile and the checked call path."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import edge_add_cases as cases
import edgeadd_mirror
from util import StubLib, f64_at, i64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
M64 = (1 << 64) - 1
ADD_SALT = 0x6564676561646473
OTHER_SALTS = (0x6E6F646564726F70, 0x72776C6B73616D70, 0x6564676564726F70)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return edgeadd_mirror.build(tmp_path_factory.mktemp("edgeadd"))


# ------------------------------------------------------------------------------------------------ restatements, from the prose
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u_add_int(seed, k, i, c):
    """The 53-bit integer m of the coin u_add(k, i, c) = m 2^-53."""
    return mix64(mix64(((seed + k) & M64) ^ ADD_SALT) ^ mix64((2 * i + c) & M64)) >> 11


def pick_int(m, n):
    """min((int64)(u * (double)n), n - 1) for u = m 2^-53: the product rounded once to float64, truncated, clamped."""
    return min(int(float(Fraction(m * n, 1 << 53))), n - 1)


def np_added(seed, k, count, n):
    """The added pairs of view k by the prose, vectorised: (count, 2) int64."""
    mix = lambda z: np_mix64(z)
    with np.errstate(over="ignore"):
        view = np.uint64(mix64(((seed + k) & M64) ^ ADD_SALT))
        ctr = np.arange(2 * count, dtype=np.uint64)
        u = (mix(view ^ mix(ctr)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    return np.minimum((u * float(n - 1)).astype(np.int64), n - 2).reshape(count, 2)


def np_mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def view_of(got, k):
    return got["rows"][got["ptr"][k]:got["ptr"][k + 1]], got["added"][got["aptr"][k]:got["aptr"][k + 1]]


# ------------------------------------------------------------------------------------------------ 1. the rules
def test_constants(lib):
    assert lib.edgeadd_row_tile() == cases.ROW_TILE and lib.edgeadd_max_views() == 32
    assert ADD_SALT not in OTHER_SALTS
    assert "0x%Xull" % ADD_SALT in open(os.path.join(INC, "rlap_edgeadd.h")).read()
    for n, bits in [(0, 1), (1, 1), (2, 1), (3, 2), (4, 2), (5, 3), (1024, 10), (1025, 11), (2**31 - 1, 31)]:
        assert lib.edgeadd_id_bits(n) == bits
    assert lib.edgeadd_pair_key(5, 9, 1025) == (5 << 11) | 9 and lib.edgeadd_pair_key(2**31 - 2, 2**31 - 2, 2**31 - 1) == ((2**31 - 2) << 31) | (2**31 - 2)
    # one sort for all views while the view number fits beside the key below bit 63
    assert lib.edgeadd_one_sort(2**31 - 1, 1) == 1 and lib.edgeadd_one_sort(2**31 - 1, 2) == 1 and lib.edgeadd_one_sort(2**31 - 1, 3) == 0
    assert lib.edgeadd_one_sort(2**29, 32) == 1 and lib.edgeadd_one_sort(2**29 + 1, 32) == 0 and lib.edgeadd_one_sort(5000, 3) == 1


def test_the_stride_constant_and_the_large_input(lib):
    """MAX_GRID_ROWS is what one round of a strided launch of rlap_edgeadd.hip covers, and the large input of
    tests/test_gpu_augment_strides.py is one round, one whole wave and one lane."""
    src = open(os.path.join(INC, "rlap_edgeadd.hip")).read()
    grid = int(re.search(r"constexpr int64_t EA_MAX_GRID = (\d+);", src).group(1))
    tile = int(re.search(r"constexpr int TILE = (\d+);", open(os.path.join(INC, "rlap_edgedrop.h")).read()).group(1))
    assert "constexpr int TILE = edgedrop::TILE;" in open(os.path.join(INC, "rlap_edgeadd.h")).read()
    assert "return capped_blocks(n, TILE, EA_MAX_GRID);" in src and cases.MAX_GRID_ROWS == grid * tile
    assert cases.STRIDE_E == cases.MAX_GRID_ROWS + 64 + 1 and cases.STRIDE_N > cases.STRIDE_E
    s, d, n = cases.stride_rows()
    assert s.size == d.size == cases.STRIDE_E and n == cases.STRIDE_N and max(s.max(), d.max()) < n
    assert (np.diff(s * n + d) < 0).any()                                              # the keys do not ascend: the key set is built
    assert edgeadd_mirror.counts_of(cases.STRIDE_E, 0.001) == [2097]                     # the large input's added rows
    assert edgeadd_mirror.counts_of(5000, (cases.STRIDE_E + 0.5) / 5000) == [cases.STRIDE_E]   # ... and the many added rows of a small one


def test_the_key_set_model_and_its_wrapping_inputs(lib):
    """The model of tests/edge_add_cases.py restates the device's key set (2 E slots, home = mix64(key) % slots, linear probing that
    wraps).  Among the tiny inputs it picks, the occupied slots cross the table's end, and among the added keys of the calls the GPU
    suite makes with them, probes cross that end both ways: one finds its key beyond it, one finds an empty slot beyond it."""
    src = open(os.path.join(INC, "rlap_edgeadd.hip")).read()
    assert "a.slots = g.coalesce ? 2 * E : 0;" in src and "return (int64_t)(mix64(key) % (uint64_t)a.slots);" in src
    assert src.count("h = h + 1 == a.slots ? 0 : h + 1;") == 2                           # the insertion and the probe
    assert cases.mix64(12345) == mix64(12345)
    for n in (2, 3, 4, 5, 6, 1025):
        assert cases.id_bits(n) == lib.edgeadd_id_bits(n)
        assert cases.pair_keys([n - 1, 1], [0, n - 1], n) == [lib.edgeadd_pair_key(n - 1, 0, n), lib.edgeadd_pair_key(1, n - 1, n)]
    unsorted, found_across, empty_across = 0, 0, 0
    seeds = cases.wrapping_inputs()
    for seed in cases.WRAP_SEEDS:
        s, d, n = cases.tiny_unsorted(seed)
        assert 2 <= s.size <= 12 and 3 <= n <= 6
        keys = cases.pair_keys(s, d, n)
        ascending = all(a <= b for a, b in zip(keys, keys[1:]))
        unsorted += 0 if ascending else 1
        if seed not in seeds:
            continue
        got = edgeadd_mirror.run(lib, s, d, n, w=cases.weights(s.size), ratio=cases.WRAP_RATIOS, seed=cases.SEED)
        assert got["input_sorted"] == 0 and not ascending
        table, wrapped = cases.table_of(keys)
        assert wrapped and sorted(k for k in table if k is not None) == sorted(set(keys)) and len(table) == 2 * s.size
        assert cases.table_of(keys[::-1])[1] and [k is None for k in cases.table_of(keys[::-1])[0]] == [k is None for k in table]   # any order: the same slots
        for key in sorted(set(cases.pair_keys(got["added"][:, 0], got["added"][:, 1], n))):
            found, crossed = cases.probe(table, key)
            assert found == (key in keys)
            found_across += 1 if crossed and found else 0
            empty_across += 1 if crossed and not found else 0
        for k in range(len(cases.WRAP_RATIOS)):                                          # the counts the device takes from the set are the mirror's
            rows, added = view_of(got, k)
            fresh = sum(1 for key in set(cases.pair_keys(added[:, 0], added[:, 1], n)) if not cases.probe(table, key)[0])
            assert rows.shape[0] == got["input_distinct"] + fresh
    print(f"{unsorted} inputs whose keys do not ascend, {len(seeds)} whose table wraps; probes across the end: {found_across} find their key, {empty_across} an empty slot")
    assert len(seeds) >= 20 and found_across >= 1 and empty_across >= 1


def test_draws_bit_for_bit(lib):
    for seed, k, i, c in [(0, 0, 0, 0), (0, 0, 0, 1), (0, 1, 0, 0), (20, 0, 1, 0), (20, 31, 12345, 1), (2**64 - 1, 1, 2**31 - 3, 1), (2**63 + 5, 7, 4097, 0)]:
        assert lib.edgeadd_u_add(seed, k, i, c) == u_add_int(seed, k, i, c) * 2.0 ** -53
        for n in (2, 3, 7, 513, 2**31 - 1):
            got = lib.edgeadd_draw(seed, k, i, c, n)
            assert got == pick_int(u_add_int(seed, k, i, c), n - 1) and 0 <= got <= n - 2
    assert u_add_int(3, 0, 1, 0) == u_add_int(3, 0, 0, 2)                              # the counter is 2 i + c, nothing else
    assert u_add_int(3, 0, 1, 0) != u_add_int(3, 1, 1, 0) and u_add_int(3, 1, 1, 0) == u_add_int(4, 0, 1, 0)   # view k of seed: seed + k


def test_no_draw_reaches_the_last_node_and_every_other_id_occurs(lib):
    """The reference's randint(0, num_nodes - 1) has an exclusive upper end: ids lie in [0, N - 2].  300,000 draws on N = 12: every id
    of [0, 10] occurs, 11 never does, and the counts are uniform within 5 standard deviations (a fixed seed: deterministic)."""
    n, count = 12, 150000
    empty = np.zeros(0, dtype=np.int64)
    got = edgeadd_mirror.run(lib, empty, empty, n, num_add=[count], seed=cases.SEED)
    added = got["added"]
    assert np.array_equal(added, np_added(cases.SEED, 0, count, n))
    hist = np.bincount(added.ravel(), minlength=n)
    q = 1.0 / (n - 1)
    print(f"draw counts on N = {n}: {hist.tolist()}; expected {2 * count * q:.0f} +- {5 * np.sqrt(2 * count * q * (1 - q)):.0f}")
    assert hist[n - 1] == 0 and (hist[:n - 1] > 0).all() and (np.abs(hist[:n - 1] - 2 * count * q) <= 5 * np.sqrt(2 * count * q * (1 - q))).all()
    two = edgeadd_mirror.run(lib, empty, empty, 2, num_add=[500], seed=1)
    assert not two["added"].any() and two["rows"].tolist() == [[0.0, 0.0, 500.0]]       # N = 2: every added row is (0, 0)


@pytest.mark.parametrize("ratio", [0.1, 0.3, 1 / 3, 0.7, 2.5, 0.0, 1.0])
def test_counts_are_the_references_expression(lib, ratio):
    from rlap_amd import ops
    for E in (0, 1, 3, 10, 700, 2049, 10**6 + 3):
        assert edgeadd_mirror.counts_of(E, ratio) == [int(E * ratio)]
        assert ops._add_args(torch.zeros((2, E), dtype=torch.int64), None, 5, ratio, 0)[2] == [int(E * ratio)]
    src, dst, n = cases.graph("messy")
    got = edgeadd_mirror.run(lib, src, dst, n, ratio=ratio)
    assert got["added"].shape[0] == int(700 * ratio) and got["aptr"].tolist() == [0, int(700 * ratio)]


@pytest.mark.parametrize("name", list(cases.GRAPHS))
def test_structure_against_numpy(lib, name):
    src, dst, n = cases.graph(name)
    E = src.size
    for w, exact in ((None, True), (cases.dyadic(E), True), (cases.weights(E), False)):
        got = edgeadd_mirror.run(lib, src, dst, n, w=w, ratio=(0.3, 2.5), seed=cases.SEED)
        assert got["ptr"][0] == 0 and got["aptr"].tolist() == [0, int(E * 0.3), int(E * 0.3) + int(E * 2.5)]
        assert got["input_distinct"] == np.unique(src * n + dst).size
        for k in range(2):
            rows, added = view_of(got, k)
            assert np.array_equal(added, np_added(cases.SEED, k, added.shape[0], n))
            s, t = np.concatenate([src, added[:, 0]]), np.concatenate([dst, added[:, 1]])
            keys, inv, mult = np.unique(s * n + t, return_inverse=True, return_counts=True)
            assert np.array_equal(rows[:, 0] * n + rows[:, 1], keys)                  # strictly ascending, every input pair present
            if w is None:
                assert np.array_equal(rows[:, 2], mult.astype(np.float64))            # the multiplicity coalesce computes
            elif exact:
                want = np.zeros(keys.size)
                np.add.at(want, inv, np.concatenate([w, np.ones(added.shape[0])]))
                assert np.array_equal(rows[:, 2], want)
            assert np.array_equal(rows, cases.python_reference(src, dst, w, added, n))   # input order, then the count once


def test_a_long_run_is_summed_in_input_order(lib):
    E = 2 * cases.T + 5
    src, dst = np.full(E, 3, dtype=np.int64), np.full(E, 1, dtype=np.int64)
    w = cases.weights(E)
    got = edgeadd_mirror.run(lib, src, dst, 9, w=w, ratio=0.0)
    s = 0.0
    for v in w.tolist():
        s += v
    assert got["rows"].tolist() == [[3.0, 1.0, s]] and s != float(np.sum(w[::-1])) and got["input_distinct"] == 1


def test_uncoalesced_is_the_plain_concatenation(lib):
    src, dst, n = cases.graph("messy")
    w = cases.weights(src.size)
    got = edgeadd_mirror.run(lib, src, dst, n, w=w, ratio=(0.3, 0.4), seed=cases.SEED, coalesce=False)
    assert got["ptr"].tolist() == [0, 700 + 210, 1400 + 210 + 280]
    for k in range(2):
        rows, added = view_of(got, k)
        assert np.array_equal(added, np_added(cases.SEED, k, added.shape[0], n))
        want = np.concatenate([np.stack([src, dst, w], 1), np.concatenate([added, np.ones((added.shape[0], 1))], 1)])
        assert np.array_equal(rows, want)


def test_views_equal_one_view_calls(lib):
    src, dst, n = cases.graph("ba300")
    w = cases.weights(src.size)
    ratios = [0.2, 2.5, 0.0, 0.35]
    for coalesce in (True, False):
        many = edgeadd_mirror.run(lib, src, dst, n, w=w, ratio=ratios, seed=40, coalesce=coalesce)
        for k, r in enumerate(ratios):
            one = edgeadd_mirror.run(lib, src, dst, n, w=w, ratio=r, seed=40 + k, coalesce=coalesce)
            rows, added = view_of(many, k)
            assert np.array_equal(one["rows"], rows) and np.array_equal(one["added"], added)


def test_sortedness_orders_and_refusals(lib):
    src, dst, n = cases.graph("messy")
    cs, cd = cases.coalesced(src, dst, n)
    assert edgeadd_mirror.run(lib, cs, cd, n)["input_sorted"] == 1 and edgeadd_mirror.run(lib, src, dst, n)["input_sorted"] == 0
    order = np.lexsort((cs, cd))                                                        # (target, source) order, as the elimination emits
    a, b = edgeadd_mirror.run(lib, cs, cd, n, seed=2), edgeadd_mirror.run(lib, cs[order], cd[order], n, seed=2)
    assert b["input_sorted"] == 0 and np.array_equal(a["rows"], b["rows"])
    empty = np.zeros(0, dtype=np.int64)
    got = edgeadd_mirror.run(lib, empty, empty, 0, ratio=(0.5, 0.5))
    assert got["rows"].shape == (0, 3) and got["ptr"].tolist() == [0, 0, 0]
    for kw, status in [(dict(num_add=[1] * 33), 9), (dict(num_add=[-1]), 3), (dict(num_add=[2**31 - 1 - 700]), 9)]:
        with pytest.raises(edgeadd_mirror.Refused) as e:
            edgeadd_mirror.run(lib, src, dst, n, **kw)
        assert e.value.status == status, kw
    with pytest.raises(edgeadd_mirror.Refused) as e:
        edgeadd_mirror.run(lib, src, dst, n - 1)
    assert e.value.status == 2
    for nodes in (0, 1):
        with pytest.raises(edgeadd_mirror.Refused) as e:
            edgeadd_mirror.run(lib, empty, empty, nodes, num_add=[1])
        assert e.value.status == 3


# ------------------------------------------------------------------------------------------------ 2. the sanitizer program
def test_the_mirror_under_asan_and_ubsan(tmp_path):
    """The mirror as a stand-alone program with its own main: a plain executable, nothing preloaded.  Its last inputs are malformed
    (ids out of range, 33 views, a negative count, added rows without two nodes, 2^31 rows): it reports the refusals and exits clean."""
    exe = tmp_path / "edgeadd_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", INC, "-o", str(exe), edgeadd_mirror.MAIN])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": ok (") == 6 * 3 * 2 + 6 and "FAILED" not in r.stdout and "0 failures" in r.stdout
    assert r.stdout.count("refused as expected") == 9


# ------------------------------------------------------------------------------------------------ 3. the entry points
SIGS = {
    "rlap_edge_add": "h src dst w E n num_add K seed flags rows cap ptr added aptr info",
    "rlap_snapshot_plan_bytes": "m S G n flags bytes",
    "rlap_edge_plan_build": "h sc m ptr S node_ptr G n flags fill plan plan_bytes desc info",
}
ARENA = 777


class AddStub(StubLib):
    """Every view: the input rows (their weights doubled, to tell a result from an input), then one row (0, 0, 1) per added row."""

    def __init__(self):
        super().__init__(SIGS)
        from rlap_amd import _lib
        self._lib = _lib

    def export(self, name, a):
        if name == "rlap_snapshot_plan_bytes":
            self.calls.append((name, {}))
            a["bytes"]._obj.value = 4096
            return 0
        if name == "rlap_edge_plan_build":
            self.calls.append((name, {k: a[k] for k in ("m", "S", "G", "n", "flags")} | {"ptr": i64_at(a["ptr"], a["S"] + 1)}))
            d = a["desc"]._obj
            d.m, d.segments, d.graphs, d.num_nodes, d.flags, d.magic, d.plan_bytes = a["m"], a["S"], a["G"], a["n"], a["flags"], self._lib.PLAN_MAGIC, 1024
            return 0
        E, K = a["E"], a["K"]
        rec = {k: a[k] for k in ("E", "n", "K", "seed", "flags", "cap")}
        rec["num_add"] = list(a["num_add"])
        rec["src"] = i64_at(a["src"], E) if E else a["src"]
        rec["dst"] = i64_at(a["dst"], E) if E else a["dst"]
        rec["w"] = None if a["w"] is None else f64_at(a["w"], E)
        rec["has"] = tuple(a[k] is not None for k in ("added", "aptr"))
        self.calls.append((name, rec))
        if self.status:
            return self.status
        rows = ctypes.cast(a["rows"], ctypes.POINTER(ctypes.c_double)) if a["rows"] else None
        ptr = ctypes.cast(a["ptr"], ctypes.POINTER(ctypes.c_int64))
        pos = 0
        for k in range(K):
            ptr[k] = pos
            for e in range(E):
                rows[3 * pos], rows[3 * pos + 1], rows[3 * pos + 2] = rec["src"][e], rec["dst"][e], 2.0 * rec["w"][e] if rec["w"] is not None else 1.0
                pos += 1
            for _ in range(rec["num_add"][k]):
                rows[3 * pos], rows[3 * pos + 1], rows[3 * pos + 2] = 0.0, 0.0, 1.0
                pos += 1
        ptr[K] = pos
        if a["added"]:
            ctypes.memset(a["added"], 0, 16 * sum(rec["num_add"]))
            ap = ctypes.cast(a["aptr"], ctypes.POINTER(ctypes.c_int64))
            for k in range(K + 1):
                ap[k] = sum(rec["num_add"][:k])
        info = a["info"]._obj
        info.rows_needed, info.added, info.arena_bytes, info.launches, info.host_syncs, info.sorts, info.input_sorted = pos, sum(rec["num_add"]), ARENA, 9, 1, 1, 1
        return 0


@pytest.fixture
def stub(monkeypatch):
    return stub_ops(monkeypatch, AddStub())


EI = torch.tensor([[2, 0, 2, 0, 3], [0, 1, 2, 1, 2]])


def test_add_edges_arguments(stub):
    from rlap_amd import ops
    rows, ptr = ops.add_edges(EI)
    (name, b), = stub.exports()
    assert name == "rlap_edge_add" and (b["E"], b["n"], b["K"], b["num_add"], b["seed"], b["flags"], b["cap"]) == (5, 4, 1, [2], 0, 1, 7)   # max id + 1
    assert b["src"] == [2, 0, 2, 0, 3] and b["dst"] == [0, 1, 2, 1, 2] and b["w"] is None and b["has"] == (False, False)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (7, 3) and ptr.tolist() == [0, 7]
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["arena_bytes"] == ARENA and ops.last_stats["rows_needed"] == 7
    assert {"added", "input_distinct", "input_sorted", "sorts", "launches"} <= set(ops.last_stats)
    w = torch.tensor([0.5, 0.25, 2.0, 4.0, 1.5], dtype=torch.float32)
    rows, ptr, added, aptr = ops.add_edges(EI.int(), w, 9, [0.3, 2.5, 0.0], -1, coalesce=False, return_added=True)
    b = stub.exports()[-1][1]
    assert (b["n"], b["K"], b["num_add"], b["seed"], b["flags"], b["cap"]) == (9, 3, [1, 12, 0], 2**64 - 1, 0, 15 + 13)
    assert b["w"] == [0.5, 0.25, 2.0, 4.0, 1.5] and b["has"] == (True, True)
    assert tuple(rows.shape) == (28, 3) and ptr.tolist() == [0, 6, 23, 28] and rows[:5, 2].tolist() == [1.0, 0.5, 4.0, 8.0, 3.0]
    assert added.dtype == torch.int64 and tuple(added.shape) == (13, 2) and aptr.tolist() == [0, 1, 13, 13]
    rows, ptr = ops.add_edges(torch.zeros((2, 0), dtype=torch.int64), ratio=[0.5, 0.5])
    b = stub.exports()[-1][1]
    assert (b["E"], b["n"], b["src"], b["cap"], b["num_add"]) == (0, 0, None, 0, [0, 0]) and tuple(rows.shape) == (0, 3) and ptr.tolist() == [0, 0, 0]
    for r, want in [(np.float32(0.5), [2]), (torch.tensor(0.4), [2]), (np.array([0.2, 0.6]), [1, 3]), (torch.tensor([0.2, 1.0, 3.0]), [1, 5, 15]),
                    (1, [5]), (iter([0.5]), [2]), ((np.float64(0.7), 0), [3, 0])]:
        ops.add_edges(EI, ratio=r)
        assert stub.exports()[-1][1]["num_add"] == want


def test_host_checks_launch_nothing(stub):
    from rlap_amd import ops
    one = torch.tensor([[0, 0], [0, 0]])
    for args, kw, msg in [((EI.double(),), {}, "edge_index"), ((EI[0],), {}, "edge_index"), ((torch.zeros((3, 2), dtype=torch.int64),), {}, "edge_index"),
                          ((EI, torch.ones(3)), {}, "edge_weight"), ((EI, torch.ones(5, dtype=torch.int64)), {}, "edge_weight"),
                          ((EI,), dict(num_nodes=-2), "num_nodes"), ((EI,), dict(num_nodes=2.5), "num_nodes"),
                          ((EI,), dict(ratio=-0.1), "ratio"), ((EI,), dict(ratio=[0.5, float("nan")]), "ratio"), ((EI,), dict(ratio=float("inf")), "ratio"),
                          ((EI,), dict(ratio=[0.5] * 33), "ratio"), ((EI,), dict(ratio=[]), "ratio"), ((EI,), dict(ratio="0.5"), "ratio"),
                          ((EI,), dict(ratio=True), "ratio"), ((EI,), dict(ratio=None), "ratio"), ((EI,), dict(ratio=2.0**31), "ratio"),
                          ((one, None, 1), dict(ratio=0.5), "num_nodes"), ((one,), dict(ratio=0.5), "num_nodes"),     # N < 2 with a row to add
                          ((EI,), dict(seed=1.5), "seed"), ((EI,), dict(seed="7"), "seed")]:
        with pytest.raises(ValueError, match=msg):
            ops.add_edges(*args, **kw)
    assert stub.exports() == [] and ops.last_stats is None
    ops.add_edges(one, None, 1, ratio=0.4)                                              # N = 1 without a row to add is a call
    assert stub.exports()[-1][1]["num_add"] == [0]


@pytest.mark.parametrize("status,error,text", [(2, ValueError, "status 2"), (3, ValueError, "status 3"), (9, RuntimeError, "status 9"),
                                               (13, RuntimeError, "status 13")])
def test_device_statuses(stub, status, error, text):
    from rlap_amd import ops
    stub.status = status
    with pytest.raises(error, match=text):
        ops.add_edges(EI)
    assert ops.last_stats is None and [c[0] for c in stub.exports()] == ["rlap_edge_add"]


def test_seeds_none_draws_per_call_an_integer_repeats(stub):
    from rlap_amd import adapters, ops
    x = torch.ones(4, 3)
    seeds = lambda: [c[1]["seed"] for c in stub.exports() if c[0] == "rlap_edge_add"]
    aug1, aug2 = adapters.EdgeAdding(0.5), adapters.EdgeAdding(0.5)
    aug1(x, EI), aug2(x, EI), aug1(x, EI), aug2.augment((x, EI, None))
    assert len(set(seeds())) == 4 and aug1.last_seed == seeds()[2] and aug2.last_seed == seeds()[3]
    fixed = adapters.EdgeAdding(0.5, seed=11)
    fixed(x, EI), fixed(x, EI)
    assert seeds()[-2:] == [11, 11] and fixed.last_seed == 11
    stub.calls.clear()
    views = adapters.EdgeAddingViews((0.5, 0.5))
    for _ in range(2):                                                              # two steps of the (aug1, aug2) pair: one call a step
        for aug in views.augmentors():
            aug(x, EI)
    views.augment((x, EI, None)), views.plan((x, EI, None))
    assert len(seeds()) == 4 and len(set(seeds())) == 4 and views.last_seed == seeds()[-1]
    assert all(abs(a - b) > 1 for a in seeds() for b in seeds() if a != b)           # view k uses seed + k: no view shares another call's coins
    fixed = adapters.EdgeAddingViews((0.3, 0.3), seed=5)
    fixed.augment((x, EI, None)), fixed.augment((x, EI, None))
    assert seeds()[-2:] == [5, 5]
    torch.manual_seed(3)
    ops.add_edges(EI, seed=None)
    first = seeds()[-1]
    ops.add_edges(EI, seed=None)
    torch.manual_seed(3)
    ops.add_edges(EI, seed=None)
    assert seeds()[-2] != first and seeds()[-1] == first and 0 <= first < 2**62      # from torch's RNG: reproducible under manual_seed
    with pytest.raises(ValueError, match="pes"):
        adapters.EdgeAddingViews(())


def test_adapters_reach_the_call(stub):
    from rlap_amd import adapters
    x = torch.ones(6, 3, dtype=torch.float64)
    w = torch.tensor([0.5, 0.25, 2.0, 4.0, 1.5], dtype=torch.float64)
    aug = adapters.EdgeAdding(0.5)
    g = aug(x, EI, w)
    b = stub.exports()[-1][1]
    assert (b["n"], b["K"], b["num_add"], b["flags"]) == (4, 1, [2], 1)                 # max id + 1, as the reference; coalesced
    assert g.x is x and g.edge_index.dtype == torch.int64 and tuple(g.edge_index.shape) == (2, 7) and torch.equal(g.edge_index[:, :5], EI)
    assert g.edge_weights.tolist() == [1.0, 0.5, 4.0, 8.0, 3.0, 1.0, 1.0]                # the call's weights, one per edge of the result
    g = aug.augment((x, EI, None))
    assert g.edge_weights is None and tuple(g.edge_index.shape) == (2, 7)               # an unweighted input stays unweighted
    views = adapters.EdgeAddingViews((0.3, 0.7), 5)
    graphs = views.augment(adapters.Graph(x, EI, w))
    b = stub.exports()[-1][1]
    assert (b["num_add"], b["seed"], b["K"], b["n"]) == ([1, 3], 5, 2, 6) and len(graphs) == 2
    assert tuple(graphs[0].edge_index.shape) == (2, 6) and tuple(graphs[1].edge_index.shape) == (2, 8) and graphs[1].edge_weights.shape[0] == 8
    before = len(stub.exports())
    aug1, aug2 = views.augmentors()
    g1, g2 = aug1(x, EI, w), aug2(x, EI, w)
    assert len(stub.exports()) == before + 1 and tuple(g1.edge_index.shape) == (2, 6) and tuple(g2.edge_index.shape) == (2, 8)   # the pair shares one call
    aug1(x, EI, w)
    assert len(stub.exports()) == before + 2
    plan = adapters.EdgeAddingViews((0.3, 0.7)).plan(adapters.Graph(x, EI, None), directions="forward")
    names = [c[0] for c in stub.exports()[-3:]]
    assert names == ["rlap_edge_add", "rlap_snapshot_plan_bytes", "rlap_edge_plan_build"]
    b = stub.exports()[-1][1]
    assert (b["m"], b["S"], b["G"], b["n"], b["flags"], b["ptr"]) == (14, 2, 1, 6, 2 | 4 | 256, [0, 6, 14]) and plan.layers == 2


def test_layout_matches_the_header(tmp_path):
    """_lib.EdgeAddInfo and rlap_edge_add_info describe the same bytes (the check of tests/test_cabi_symbols.py's LAYOUTS)."""
    from rlap_amd import _lib
    cls, c_name = _lib.EdgeAddInfo, "rlap_edge_add_info"
    fields = [f for f, _ in cls._fields_]
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    end = hdr.index("} %s;" % c_name)
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    declared = [name for decl in re.findall(r"\b(?:int32_t|int64_t|float|double)\s+([a-z_0-9, ]+);", body) for name in decl.split(", ")]
    assert declared == fields == ["rows_needed", "added", "input_distinct", "launches", "arena_bytes", "input_sorted", "sorts", "host_syncs", "pad"]
    src = tmp_path / "layout.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rlap_hip.h"', "int main(void) {", f'    printf("sizeof %zu\\n", sizeof({c_name}));']
    lines += [f'    printf("{f} %zu\\n", offsetof({c_name}, {f}));' for f in fields] + ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(cls) and ctypes.sizeof(cls) % 8 == 0
    assert {f: int(v) for f, v in got.items()} == {f: getattr(cls, f).offset for f in fields}


def test_export_in_header_exports_makefile_and_the_checked_call_path():
    from rlap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "rlap_edge_add" in _lib.EXPORTS and re.search(r"\bint rlap_edge_add\(rlap_handle h, const int64_t\* d_src", hdr)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rlap_edge_add")
    api = open(os.path.join(INC, "rlap_api.hip")).read()
    body = api[api.index("int rlap_edge_add("):api.index("int rlap_edge_drop(")]
    assert "poisoned_call(h," in body and "edge_add_run(" in body and "hipMalloc" not in body and "RLAP_E_TOO_LARGE" in body
    assert "h_num_add" in body and "ratio" not in body                                  # the C ABI takes the counts, never the ratios
    assert all(out in body[body.index("poisoned_call(h,"):] for out in ("d_rows", "d_ptr", "d_added", "d_aptr"))   # all four poisoned
    src = open(os.path.join(INC, "rlap_edgeadd.hip")).read()
    assert "hipMalloc" not in src and "asm" not in src and not re.search(r"atomic\w*\([^;]*(double|float)", src)
    assert src.count("hipStreamSynchronize(") == 2                                      # one in the coalesced path, one in the plain one
    assert '#include "rlap_edgeadd.h"' in src and '#include "rlap_edgeadd.h"' in open(edgeadd_mirror.SRC).read()   # one set of rules
    assert '#include "rlap_rowcompact_dev.h"' in src and "#define" not in src           # the launch macro, clamp, store_row, scan_tmp_bytes: the shared ones
    mk = open(os.path.join(INC, "Makefile")).read()
    assert "rlap_edgeadd.o" in mk and "rlap_edgeadd.h" in mk and "-ffp-contract=off" in mk and "fast-math" not in mk
    import inspect
    from rlap_amd import ops
    assert '_device_call("rlap_edge_add"' in inspect.getsource(ops.add_edges)
