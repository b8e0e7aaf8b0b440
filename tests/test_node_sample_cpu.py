"""Node dropping and random-walk subgraph views without a GPU (rlap_node_sample, ops.sample_subgraphs).

1. The rules of rlap_amd/csrc/rlap_nodesample.h -- compiled here with g++ through tests/csrc/nodesample_mirror.cc, the same
   functions rlap_nodesample.hip's kernels read -- against restatements written from the prose of the rules alone: both coins and
   the pick in pure-Python integers and fractions, the drop set and its rows in numpy, the walks in Python over outgoing lists
   built with a stable argsort.  Everything is compared by equality.
2. The mirror as a stand-alone program under -fsanitize=address,undefined, malformed inputs included.
3. The Python -> C mapping of ops.sample_subgraphs and the adapters on a stub library, every ValueError raised before the device is
   touched, the layout of rlap_node_sample_info, and the export's place in the header, _lib.EXPORTS, the Makefile and the checked
   call path."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

import node_sample_cases as cases
import nodesample_mirror
from util import StubLib, f64_at, i64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
M64 = (1 << 64) - 1
NODE_SALT, WALK_SALT, EDGE_SALT = 0x6E6F646564726F70, 0x72776C6B73616D70, 0x6564676564726F70


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return nodesample_mirror.build(tmp_path_factory.mktemp("nodesample"))


# ------------------------------------------------------------------------------------------------ restatements, from the prose
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def coin_int(view, row):
    """The 53-bit integer m of a coin u = m 2^-53."""
    return mix64(view ^ row) >> 11


def u_node_int(seed, k, v):
    return coin_int(mix64(((seed + k) & M64) ^ NODE_SALT), mix64(v))


def u_walk_int(seed, k, i, t, L):
    return coin_int(mix64(((seed + k) & M64) ^ WALK_SALT), mix64((i * (L + 1) + t) & M64))


def pick_int(m, n):
    """min((int64)(u * (double)n), n - 1) for u = m 2^-53: the product rounded once to float64 (Fraction -> float rounds to nearest
    even), truncated, clamped."""
    return min(int(float(Fraction(m * n, 1 << 53))), n - 1)


def np_mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def np_drop_sets(seed, ps, n):
    """(K, n) bool: node v is in view k iff u_node(k, v) >= p[k]."""
    with np.errstate(over="ignore"):
        nodes = np_mix64(np.arange(n, dtype=np.uint64))
        u = [(np_mix64(np.uint64(mix64(((seed + k) & M64) ^ NODE_SALT)) ^ nodes) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 for k in range(len(ps))]
    return np.stack([u[k] >= ps[k] for k in range(len(ps))]).reshape(len(ps), n)


def np_rows(src, dst, w, sets):
    """The rows whose two ends are in the set (np.isin on both endpoints), view-major, in input order."""
    parts, ptr = [], [0]
    for s in sets:
        ids = np.flatnonzero(s)
        m = np.isin(src, ids) & np.isin(dst, ids)
        parts.append(np.stack([src[m], dst[m], w[m] if w is not None else np.ones(int(m.sum()))], 1))
        ptr.append(ptr[-1] + int(m.sum()))
    return np.concatenate(parts).reshape(-1, 3), ptr


def py_walks(src, dst, n, seed, k, walkers, L):
    """Walks by the prose: outgoing lists in input order (a stable argsort by source), a sink keeps its walker."""
    order = np.argsort(src, kind="stable")
    tg = dst[order]
    lo = np.searchsorted(src[order], np.arange(n), "left")
    hi = np.searchsorted(src[order], np.arange(n), "right")
    out = np.zeros((walkers, L + 1), dtype=np.int64)
    for i in range(walkers):
        v = pick_int(u_walk_int(seed, k, i, 0, L), n)
        out[i, 0] = v
        for t in range(1, L + 1):
            d = int(hi[v] - lo[v])
            if d:
                v = int(tg[lo[v] + pick_int(u_walk_int(seed, k, i, t, L), d)])
            out[i, t] = v
    return out


def sets_of(walks, firsts, n):
    sets = np.zeros((len(firsts) - 1, n), dtype=bool)
    for k in range(len(firsts) - 1):
        sets[k, np.unique(walks[firsts[k]:firsts[k + 1]])] = True
    return sets


# ------------------------------------------------------------------------------------------------ 1. the rules
def test_constants(lib):
    assert lib.nodesample_row_tile() == cases.ROW_TILE and lib.nodesample_max_views() == 32 and lib.nodesample_max_walk_length() == 1024
    assert len({NODE_SALT, WALK_SALT, EDGE_SALT}) == 3
    hdr = open(os.path.join(INC, "rlap_nodesample.h")).read()
    assert "0x%Xull" % NODE_SALT in hdr and "0x%Xull" % WALK_SALT in hdr
    assert "0x%Xull" % EDGE_SALT in open(os.path.join(INC, "rlap_edgedrop.h")).read()      # COIN_SALT: the edge views' stream


def test_the_stride_constant_and_the_large_input(lib):
    """MAX_GRID_ROWS is what one round of a strided launch of rlap_nodesample.hip covers; the large input of
    tests/test_gpu_augment_strides.py is one round, one whole wave and one lane, and its node masks and bitmaps need further rounds."""
    src = open(os.path.join(INC, "rlap_nodesample.hip")).read()
    grid = int(re.search(r"constexpr int64_t NS_MAX_GRID = (\d+);", src).group(1))
    tile = int(re.search(r"constexpr int TILE = (\d+);", open(os.path.join(INC, "rlap_edgedrop.h")).read()).group(1))
    assert "constexpr int TILE = edgedrop::TILE;" in open(os.path.join(INC, "rlap_nodesample.h")).read()
    assert "return capped_blocks(n, TILE, NS_MAX_GRID);" in src and cases.MAX_GRID_ROWS == grid * tile
    assert "capped_blocks(W, TILE / WAVE, NS_MAX_GRID)" in src                            # k_ns_drop_bits: a word a wave, 4 words a workgroup
    assert cases.STRIDE_E == cases.MAX_GRID_ROWS + 64 + 1
    assert (cases.STRIDE_N + 63) // 64 > grid * (tile // 64) and len(cases.PS) * cases.STRIDE_N > cases.MAX_GRID_ROWS


@pytest.mark.parametrize("n", cases.TOP_ID_NODES)
def test_walks_pass_through_the_top_id(lib, n):
    """The condition the GPU suite leans on: with these rows and this many walkers, walks start on id n - 1, arrive at it from
    another node and leave it, so its bit -- bit 0 of a bitmap word of its own -- is set, tested and walked from."""
    src, dst, _ = cases.top_id_rows(n)
    assert (n - 1) % 64 == 0 and (src == n - 1).sum() >= 3 and (dst == n - 1).sum() >= 4
    got = nodesample_mirror.run(lib, src, dst, n, **cases.top_id_walk(n))
    assert cases.passes_through(got["walks"], n - 1) == (True, True, True)
    assert got["nodes"][0, n - 1] and got["rows"].shape[0] > 0


def test_coins_bit_for_bit(lib):
    for seed, k, v in [(0, 0, 0), (0, 1, 0), (20, 0, 1), (20, 31, 12345), (2**64 - 1, 1, 2**31 - 1), (2**63 + 5, 7, 4097), (7, 3, 63)]:
        assert lib.nodesample_u_node(seed, k, v) == u_node_int(seed, k, v) * 2.0 ** -53
    for seed, k, i, t, L in [(0, 0, 0, 0, 0), (0, 0, 0, 0, 10), (20, 1, 5, 3, 10), (20, 31, 2**31 - 2, 1024, 1024), (2**64 - 1, 1, 257, 1, 1),
                             (2**63 + 5, 7, 64, 10, 10), (3, 0, 1, 0, 10), (3, 0, 0, 11, 11)]:
        assert lib.nodesample_u_walk(seed, k, i, t, L) == u_walk_int(seed, k, i, t, L) * 2.0 ** -53
    assert u_walk_int(3, 0, 1, 0, 10) == u_walk_int(3, 0, 0, 11, 11)                      # the counter is i (L + 1) + t, nothing else
    us = np.array([lib.nodesample_u_node(cases.SEED, 0, v) for v in range(2000)])
    assert 0.0 <= us.min() and us.max() < 1.0 and abs(us.mean() - 0.5) < 0.05
    assert lib.nodesample_u_node(5, 0, 9) != lib.nodesample_u_walk(5, 0, 0, 9, 10)        # two salts: two streams


def test_pick_bit_for_bit(lib):
    top = (1 << 53) - 1
    for n in (1, 2, 3, 2**31 - 1):
        assert lib.nodesample_pick(top * 2.0 ** -53, n) == pick_int(top, n) == n - 1      # the largest u, (2^53 - 1) 2^-53
        # the rounded product stays below n for every n < 2^53 (n 2^-53 is at least half a unit in the last place below n, and the
        # tie at a power of two is exact), so the clamp is a guard that never binds: the restatement says so without it
        assert int(float(Fraction(top * n, 1 << 53))) == n - 1
    rs = np.random.RandomState(1)
    for n in (1, 2, 3, 7, 513, 4097, 2**31 - 1):
        for m in [0, 1, top, top - 1, 1 << 52] + [int(x) for x in rs.randint(0, 1 << 62, 40) >> 9]:
            got = lib.nodesample_pick(m * 2.0 ** -53, n)
            assert got == pick_int(m, n) and 0 <= got < n


@pytest.mark.parametrize("name", list(cases.GRAPHS))
def test_drop_equals_numpy(lib, name):
    src, dst, n = cases.graph(name)
    w = cases.weights(src.size)
    got = nodesample_mirror.run(lib, src, dst, n, w=w, p=cases.PS, seed=cases.SEED)
    sets = np_drop_sets(cases.SEED, cases.PS, n)
    assert np.array_equal(got["nodes"], sets)
    assert all(bool(sets[k, v]) == (u_node_int(cases.SEED, k, v) * 2.0 ** -53 >= cases.PS[k]) for k in range(2) for v in range(0, n, 7))
    rows, ptr = np_rows(src, dst, w, sets)
    assert np.array_equal(got["rows"], rows) and got["ptr"].tolist() == ptr
    keep = nodesample_mirror.run(lib, src, dst, n, p=[0.0, 1.0, 0.0], seed=3)
    E = src.size
    assert keep["nodes"][0].all() and not keep["nodes"][1].any() and keep["ptr"].tolist() == [0, E, E, 2 * E]   # p = 0: all; p = 1: none
    assert np.array_equal(keep["rows"][:E, 0], src) and np.array_equal(keep["rows"][E:, 1], dst) and (keep["rows"][:, 2] == 1.0).all()


@pytest.mark.parametrize("L", cases.WALK_LENGTHS)
def test_walks_equal_the_python_restatement(lib, L):
    src, dst, n = cases.graph("directed")
    w = cases.weights(src.size)
    for seeds in ((0, 1), (63, 64), (65, 257)):
        got = nodesample_mirror.run(lib, src, dst, n, w=w, scheme="walk", num_seeds=seeds, walk_length=L, seed=cases.SEED)
        want = np.concatenate([py_walks(src, dst, n, cases.SEED, k, s, L) for k, s in enumerate(seeds)])
        assert got["walks"].shape == (sum(seeds), L + 1) and np.array_equal(got["walks"], want)
        sets = sets_of(want, [0, seeds[0], sum(seeds)], n)
        rows, ptr = np_rows(src, dst, w, sets)
        assert np.array_equal(got["nodes"], sets) and np.array_equal(got["rows"], rows) and got["ptr"].tolist() == ptr
        if L:
            steps = want[:, :-1], want[:, 1:]
            pairs = set(zip(src.tolist(), dst.tolist()))
            out = np.bincount(src, minlength=n)
            assert all((a, b) in pairs if out[a] else a == b for a, b in zip(steps[0].ravel().tolist(), steps[1].ravel().tolist()))
    if L == 10:                                                                      # the sink, the id without rows and the hub, met
        big = nodesample_mirror.run(lib, src, dst, n, scheme="walk", num_seeds=20000, walk_length=L, seed=cases.SEED)["walks"]
        assert (big[big[:, 0] == 7] == 7).all() and (big[big[:, 0] == 9] == 9).all() and (big[:, 0] == 7).any() and (big[:, 0] == 9).any()
        after_hub = big[:, 1:][big[:, :-1] == 6]
        assert after_hub.size > 50 and np.unique(after_hub).size > 40 and set(after_hub.tolist()) <= set(range(9, 10 + cases.HUB))


def test_walk_is_uniform_over_the_outgoing_rows(lib):
    """The star's centre has 7 outgoing rows; of the walkers that start there, each neighbour gets its share within 5 standard
    deviations.  Deterministic: the seed is fixed (checked on the CPU before it was committed)."""
    src, dst, n = cases.graph("star7")
    walks = nodesample_mirror.run(lib, src, dst, n, scheme="walk", num_seeds=8 * 70000, walk_length=2, seed=cases.SEED)["walks"]
    starts = np.bincount(walks[:, 0], minlength=n)
    sd = np.sqrt(walks.shape[0] * (1 / 8) * (7 / 8))
    assert (np.abs(starts - walks.shape[0] / 8) <= 5 * sd).all()                     # the start is uniform over the nodes
    centre = walks[walks[:, 0] == 0]
    m, q = centre.shape[0], 1.0 / 7.0
    counts = np.bincount(centre[:, 1], minlength=n)
    print(f"{m} walkers start at the centre; neighbour counts {counts[1:].tolist()}, expected {m * q:.0f} +- {5 * np.sqrt(m * q * (1 - q)):.0f}")
    assert counts[0] == 0 and (np.abs(counts[1:] - m * q) <= 5 * np.sqrt(m * q * (1 - q))).all()
    assert (centre[:, 2] == centre[:, 1]).all()                                      # a leaf has no outgoing row: the walker stays
    assert (walks[walks[:, 0] != 0] == walks[walks[:, 0] != 0][:, :1]).all()


def test_views_equal_one_view_calls(lib):
    src, dst, n = cases.graph("ba300")
    many = nodesample_mirror.run(lib, src, dst, n, p=[0.2, 0.5, 0.35], seed=40)
    for k, p in enumerate([0.2, 0.5, 0.35]):
        one = nodesample_mirror.run(lib, src, dst, n, p=p, seed=40 + k)
        assert np.array_equal(one["nodes"][0], many["nodes"][k]) and np.array_equal(one["rows"], many["rows"][many["ptr"][k]:many["ptr"][k + 1]])
    seeds = [30, 0, 90]
    many = nodesample_mirror.run(lib, src, dst, n, scheme="walk", num_seeds=seeds, walk_length=4, seed=40)
    first = [0, 30, 30, 120]
    assert many["ptr"][1] == many["ptr"][2] and not many["nodes"][1].any()            # an empty view: equal offsets
    for k, s in enumerate(seeds):
        one = nodesample_mirror.run(lib, src, dst, n, scheme="walk", num_seeds=s, walk_length=4, seed=40 + k)
        assert np.array_equal(one["walks"], many["walks"][first[k]:first[k + 1]]) and np.array_equal(one["nodes"][0], many["nodes"][k])
        assert np.array_equal(one["rows"], many["rows"][many["ptr"][k]:many["ptr"][k + 1]])


def test_a_batch_never_walks_across_graphs(lib):
    src, dst, n = cases.graph("two_ba50")
    walks = nodesample_mirror.run(lib, src, dst, n, scheme="walk", num_seeds=400, walk_length=10, seed=cases.SEED)["walks"]
    side = walks >= 50
    assert (side == side[:, :1]).all() and side[:, 0].any() and not side[:, 0].all()
    assert (walks[:, 1:] != walks[:, :-1]).any()


def test_edges_of_tiles_words_and_refusals(lib):
    for E in cases.TILE_EDGE_ROWS:
        s, d, n = cases.random_rows(E)
        for K in (1, 2, 3):
            got = nodesample_mirror.run(lib, s, d, n, p=[0.3] * K, seed=cases.SEED)
            rows, ptr = np_rows(s, d, None, np_drop_sets(cases.SEED, [0.3] * K, n))
            assert np.array_equal(got["rows"], rows) and got["ptr"].tolist() == ptr
    for n in cases.WORD_EDGE_NODES:
        s, d, _ = cases.random_rows(300, n)
        assert np.array_equal(nodesample_mirror.run(lib, s, d, n, p=0.5, seed=1)["nodes"], np_drop_sets(1, [0.5], n))
        got = nodesample_mirror.run(lib, s, d, n, scheme="walk", num_seeds=n // 2 + 1, walk_length=3, seed=1)
        assert np.array_equal(got["walks"], py_walks(s, d, n, 1, 0, n // 2 + 1, 3))
    empty = np.zeros(0, dtype=np.int64)
    got = nodesample_mirror.run(lib, empty, empty, 5, scheme="walk", num_seeds=[9, 2], walk_length=6)   # no rows: every walker stays
    assert got["rows"].shape == (0, 3) and got["ptr"].tolist() == [0, 0, 0] and (got["walks"] == got["walks"][:, :1]).all()
    src, dst, n = cases.graph("ba300")
    for kw, status in [(dict(p=[0.5] * 33), 9), (dict(p=1.5), 3), (dict(p=-0.1), 3), (dict(scheme="walk", num_seeds=-1), 3),
                       (dict(scheme="walk", num_seeds=2**31), 9), (dict(scheme="walk", num_seeds=[1] * 33), 9),
                       (dict(scheme="walk", num_seeds=3, walk_length=-1), 3), (dict(scheme="walk", num_seeds=3, walk_length=1025), 3), (dict(scheme=2), 3)]:
        with pytest.raises(nodesample_mirror.Refused) as e:
            nodesample_mirror.run(lib, src, dst, n, **kw)
        assert e.value.status == status, kw
    with pytest.raises(nodesample_mirror.Refused) as e:
        nodesample_mirror.run(lib, src, dst, n - 1)
    assert e.value.status == 2
    with pytest.raises(nodesample_mirror.Refused) as e:
        nodesample_mirror.run(lib, empty, empty, 0, scheme="walk", num_seeds=1)
    assert e.value.status == 3
    assert nodesample_mirror.run(lib, empty, empty, 0, scheme="walk", num_seeds=0)["ptr"].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ 2. the sanitizer program
def test_the_mirror_under_asan_and_ubsan(tmp_path):
    """The mirror as a stand-alone program with its own main: a plain executable, nothing preloaded.  Its last inputs are malformed
    (ids out of range, 33 views, p = 1.5, walkers without nodes, 2^31 walkers): it reports the refusals and exits clean."""
    exe = tmp_path / "nodesample_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", INC, "-o", str(exe), nodesample_mirror.MAIN])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": ok (") == 1 + 3 * 6 + 6 * 3 * 2 + 6 * 2 + 2 and "FAILED" not in r.stdout and "0 failures" in r.stdout
    assert r.stdout.count("refused as expected") == 13


# ------------------------------------------------------------------------------------------------ 3. the entry points
SIGS = {
    "rlap_node_sample": "h src dst w E n scheme p seeds K walk_length seed rows cap ptr node_mask walks info",
    "rlap_snapshot_plan_bytes": "m S G n flags bytes",
    "rlap_edge_plan_build": "h sc m ptr S node_ptr G n flags fill plan plan_bytes desc info",
}
ARENA = 777


class SampleStub(StubLib):
    """Keeps every row of every view."""

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
        rec = {k: a[k] for k in ("E", "n", "scheme", "K", "walk_length", "seed", "cap")}
        rec["p"] = None if a["p"] is None else list(a["p"])
        rec["seeds"] = None if a["seeds"] is None else list(a["seeds"])
        rec["src"] = i64_at(a["src"], E) if E else a["src"]
        rec["dst"] = i64_at(a["dst"], E) if E else a["dst"]
        rec["w"] = None if a["w"] is None else f64_at(a["w"], E)
        rec["has"] = tuple(a[k] is not None for k in ("node_mask", "walks"))
        self.calls.append((name, rec))
        if self.status:
            return self.status
        rows = ctypes.cast(a["rows"], ctypes.POINTER(ctypes.c_double)) if a["rows"] else None
        ptr = ctypes.cast(a["ptr"], ctypes.POINTER(ctypes.c_int64))
        for k in range(K):
            ptr[k] = k * E
            for e in range(E):
                rows[3 * (k * E + e)], rows[3 * (k * E + e) + 1] = rec["src"][e], rec["dst"][e]
                rows[3 * (k * E + e) + 2] = rec["w"][e] if rec["w"] is not None else 1.0
        ptr[K] = K * E
        if a["node_mask"]:
            ctypes.memset(a["node_mask"], 1, K * a["n"])
        if a["walks"]:
            ctypes.memset(a["walks"], 0, 8 * sum(rec["seeds"]) * (a["walk_length"] + 1))
        info = a["info"]._obj
        info.rows_needed, info.arena_bytes, info.launches, info.host_syncs = K * E, ARENA, 5, 1
        return 0


@pytest.fixture
def stub(monkeypatch):
    return stub_ops(monkeypatch, SampleStub())


EI = torch.tensor([[2, 0, 2, 0, 3], [0, 1, 2, 1, 2]])


def test_sample_subgraphs_arguments(stub):
    from rlap_amd import ops
    rows, ptr = ops.sample_subgraphs(EI)
    (name, b), = stub.exports()
    assert name == "rlap_node_sample" and (b["E"], b["n"], b["scheme"], b["K"], b["p"], b["seeds"]) == (5, 4, 0, 1, [0.5], None)   # max id + 1
    assert (b["walk_length"], b["seed"], b["cap"]) == (0, 0, 5)
    assert b["src"] == [2, 0, 2, 0, 3] and b["dst"] == [0, 1, 2, 1, 2] and b["w"] is None and b["has"] == (False, False)
    assert rows.dtype == torch.float64 and rows.tolist() == [[2, 0, 1], [0, 1, 1], [2, 2, 1], [0, 1, 1], [3, 2, 1]] and ptr.tolist() == [0, 5]
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["arena_bytes"] == ARENA and ops.last_stats["rows_needed"] == 5
    w = torch.tensor([0.5, 0.25, 2.0, 4.0, 1.5], dtype=torch.float32)
    rows, ptr, nodes, walks = ops.sample_subgraphs(EI.int(), w, 9, "walk", 0.9, [3, 0, 2], 7, -1, return_nodes=True, return_walks=True)
    b = stub.exports()[-1][1]
    assert (b["n"], b["scheme"], b["K"], b["p"], b["seeds"], b["walk_length"], b["seed"], b["cap"]) == (9, 1, 3, None, [3, 0, 2], 7, 2**64 - 1, 15)
    assert b["w"] == [0.5, 0.25, 2.0, 4.0, 1.5] and b["has"] == (True, True)
    assert tuple(rows.shape) == (15, 3) and ptr.tolist() == [0, 5, 10, 15] and rows[5:10, 2].tolist() == [0.5, 0.25, 2.0, 4.0, 1.5]
    assert nodes.dtype == torch.bool and tuple(nodes.shape) == (3, 9) and nodes.all()
    assert walks.dtype == torch.int64 and tuple(walks.shape) == (5, 8)
    rows, ptr, nodes = ops.sample_subgraphs(EI, None, 6, "drop", (0.1, 0.2), return_nodes=True)
    b = stub.exports()[-1][1]
    assert (b["scheme"], b["p"], b["K"], b["has"]) == (0, [0.1, 0.2], 2, (True, False)) and tuple(nodes.shape) == (2, 6)
    ops.sample_subgraphs(EI, scheme="walk", num_seeds=4)
    b = stub.exports()[-1][1]
    assert (b["seeds"], b["walk_length"], b["has"]) == ([4], 10, (False, False))
    rows, ptr, walks = ops.sample_subgraphs(torch.zeros((2, 0), dtype=torch.int64), None, 3, "walk", num_seeds=[0, 0], return_walks=True)
    b = stub.exports()[-1][1]
    assert (b["E"], b["n"], b["src"], b["cap"], b["has"]) == (0, 3, None, 0, (False, False)) and tuple(rows.shape) == (0, 3) and ptr.tolist() == [0, 0, 0]
    assert tuple(walks.shape) == (0, 11)
    rows, ptr = ops.sample_subgraphs(torch.zeros((2, 0), dtype=torch.int64), p=[0.5, 0.5])
    assert stub.exports()[-1][1]["n"] == 0 and ptr.tolist() == [0, 0, 0]


def test_host_checks_launch_nothing(stub):
    from rlap_amd import ops
    none = torch.zeros((2, 0), dtype=torch.int64)
    for args, kw, msg in [((EI.double(),), {}, "edge_index"), ((EI[0],), {}, "edge_index"), ((torch.zeros((3, 2), dtype=torch.int64),), {}, "edge_index"),
                          ((EI, torch.ones(3)), {}, "edge_weight"), ((EI, torch.ones(5, dtype=torch.int64)), {}, "edge_weight"),
                          ((EI,), dict(num_nodes=-2), "num_nodes"), ((EI,), dict(num_nodes=2.5), "num_nodes"),
                          ((EI,), dict(scheme="uniform"), "scheme"), ((EI,), dict(scheme=None), "scheme"),
                          ((EI,), dict(p=1.5), "p:"), ((EI,), dict(p=[0.5, -0.1]), "p:"), ((EI,), dict(p=[0.5] * 33), "p:"), ((EI,), dict(p=[]), "p:"),
                          ((EI,), dict(p="0.5"), "p:"), ((EI,), dict(p=float("nan")), "p:"), ((EI,), dict(p=True), "p:"), ((EI,), dict(p=None), "p:"),
                          ((EI,), dict(return_walks=True), "return_walks"),
                          ((EI,), dict(scheme="walk"), "num_seeds"), ((EI,), dict(scheme="walk", num_seeds=-1), "num_seeds"),
                          ((EI,), dict(scheme="walk", num_seeds=2.0), "num_seeds"), ((EI,), dict(scheme="walk", num_seeds=[1, 0.5]), "num_seeds"),
                          ((EI,), dict(scheme="walk", num_seeds=True), "num_seeds"), ((EI,), dict(scheme="walk", num_seeds=2**31), "num_seeds"),
                          ((EI,), dict(scheme="walk", num_seeds=[1] * 33), "num_seeds"), ((EI,), dict(scheme="walk", num_seeds=[]), "num_seeds"),
                          ((EI,), dict(scheme="walk", num_seeds="3"), "num_seeds"),
                          ((EI,), dict(scheme="walk", num_seeds=3, walk_length=-1), "walk_length"),
                          ((EI,), dict(scheme="walk", num_seeds=3, walk_length=1025), "walk_length"),
                          ((EI,), dict(scheme="walk", num_seeds=3, walk_length=2.0), "walk_length"),
                          ((none,), dict(scheme="walk", num_seeds=[0, 1]), "num_seeds"), ((none, None, 0), dict(scheme="walk", num_seeds=1), "num_seeds"),
                          ((EI,), dict(seed=1.5), "seed"), ((EI,), dict(seed="7"), "seed")]:
        with pytest.raises(ValueError, match=msg):
            ops.sample_subgraphs(*args, **kw)
    assert stub.exports() == [] and ops.last_stats is None


@pytest.mark.parametrize("status,error,text", [(2, ValueError, "status 2"), (3, ValueError, "status 3"), (9, RuntimeError, "status 9"),
                                               (13, RuntimeError, "status 13")])
def test_device_statuses(stub, status, error, text):
    from rlap_amd import ops
    stub.status = status
    with pytest.raises(error, match=text):
        ops.sample_subgraphs(EI, scheme="walk", num_seeds=2)
    assert ops.last_stats is None and [c[0] for c in stub.exports()] == ["rlap_node_sample"]


def test_p_and_num_seeds_take_any_number_and_any_sequence(stub):
    from rlap_amd import ops
    for p, want in [(np.float32(0.25), [0.25]), (torch.tensor(0.25), [0.25]), (np.array(0.5), [0.5]), (1, [1.0]), (np.array([0.25, 0.5]), [0.25, 0.5]),
                    (torch.tensor([0.25, 0.5, 0.75]), [0.25, 0.5, 0.75]), ((np.float32(0.5), 0), [0.5, 0.0]), (iter([0.5]), [0.5])]:
        ops.sample_subgraphs(EI, p=p)
        assert stub.exports()[-1][1]["p"] == want
    for s, want in [(np.int32(3), [3]), (torch.tensor(3), [3]), (np.array(4), [4]), (0, [0]), (np.array([2, 5]), [2, 5]), (torch.tensor([1, 2, 3]), [1, 2, 3]),
                    ((np.int64(7), 0), [7, 0]), (iter([5]), [5]), (2**31 - 1, [2**31 - 1])]:
        ops.sample_subgraphs(EI, scheme="walk", num_seeds=s, walk_length=np.int64(3))
        assert stub.exports()[-1][1]["seeds"] == want and stub.exports()[-1][1]["walk_length"] == 3
    ops.sample_subgraphs(EI, scheme="walk", num_seeds=1, walk_length=1024)
    ops.sample_subgraphs(EI, scheme="walk", num_seeds=1, walk_length=0)
    assert stub.exports()[-1][1]["walk_length"] == 0


def test_seeds_none_draws_per_call_an_integer_repeats(stub):
    """The reference builds aug1 and aug2 with the same arguments and calls them every step: default-constructed augmentors draw a
    fresh seed per call (torch's RNG), so neither two augmentors nor two calls of one share their coins; an explicit seed is passed
    on as it is."""
    from rlap_amd import adapters, ops
    x = torch.ones(4, 3)
    seeds = lambda: [c[1]["seed"] for c in stub.exports() if c[0] == "rlap_node_sample"]
    for make in (lambda **kw: adapters.NodeDropping(0.3, **kw), lambda **kw: adapters.RWSampling(3, 5, **kw)):
        stub.calls.clear()
        aug1, aug2 = make(), make()
        aug1(x, EI), aug2(x, EI), aug1(x, EI), aug2.augment((x, EI, None))
        assert len(set(seeds())) == 4 and aug1.last_seed == seeds()[2] and aug2.last_seed == seeds()[3]
        fixed = make(seed=11)
        fixed(x, EI), fixed(x, EI)
        assert seeds()[-2:] == [11, 11] and fixed.last_seed == 11
    stub.calls.clear()
    views = adapters.NodeSampleViews("walk", (3, 3), 5)
    for _ in range(2):                                                              # two steps of the (aug1, aug2) pair: one call a step
        for aug in views.augmentors():
            aug(x, EI)
    views.augment((x, EI, None)), views.plan((x, EI, None))
    assert len(seeds()) == 4 and len(set(seeds())) == 4 and views.last_seed == seeds()[-1]
    assert all(abs(a - b) > 1 for a in seeds() for b in seeds() if a != b)           # view k uses seed + k: no view shares another call's coins
    fixed = adapters.NodeSampleViews("drop", (0.3, 0.3), seed=5)
    fixed.augment((x, EI, None)), fixed.augment((x, EI, None))
    assert seeds()[-2:] == [5, 5]
    torch.manual_seed(3)
    ops.sample_subgraphs(EI, seed=None)
    first = seeds()[-1]
    ops.sample_subgraphs(EI, seed=None)
    torch.manual_seed(3)
    ops.sample_subgraphs(EI, seed=None)
    assert seeds()[-2] != first and seeds()[-1] == first and 0 <= first < 2**62      # from torch's RNG: reproducible under manual_seed
    with pytest.raises(ValueError, match="ps_or_seeds"):
        adapters.NodeSampleViews("drop", ())


def test_adapters_reach_the_call(stub):
    from rlap_amd import adapters
    x = torch.ones(6, 3, dtype=torch.float64)
    w = torch.tensor([0.5, 0.25, 2.0, 4.0, 1.5], dtype=torch.float64)
    for aug, want in ((adapters.NodeDropping(0.3), (0, [0.3], None, 0)), (adapters.RWSampling(4), (1, None, [4], 10)), (adapters.RWSampling(4, 3), (1, None, [4], 3))):
        g = aug(x, EI, w)
        b = stub.exports()[-1][1]
        assert (b["scheme"], b["p"], b["seeds"], b["walk_length"]) == want and b["n"] == 4 and b["K"] == 1       # max id + 1, as PyGCL
        assert g.x is x and g.edge_index.dtype == torch.int64 and torch.equal(g.edge_index, EI) and torch.equal(g.edge_weights, w)
        g = aug.augment((x, EI, None))
        assert g.edge_weights is None and torch.equal(g.edge_index, EI)
    views = adapters.NodeSampleViews("walk", (3, 4), 6, 5)
    graphs = views.augment(adapters.Graph(x, EI, w))
    b = stub.exports()[-1][1]
    assert (b["scheme"], b["seeds"], b["walk_length"], b["seed"], b["K"], b["n"]) == (1, [3, 4], 6, 5, 2, 6) and len(graphs) == 2
    assert torch.equal(graphs[1].edge_index, EI)
    before = len(stub.exports())
    aug1, aug2 = views.augmentors()
    g1, g2 = aug1(x, EI, w), aug2(x, EI, w)
    assert len(stub.exports()) == before + 1 and torch.equal(g1.edge_weights, w) and torch.equal(g2.edge_index, EI)   # the pair shares one call
    aug1(x, EI, w)
    assert len(stub.exports()) == before + 2
    drop = adapters.NodeSampleViews("drop", (0.3, 0.45))
    plan = drop.plan(adapters.Graph(x, EI, None), directions="forward")
    names = [c[0] for c in stub.exports()[-3:]]
    assert names == ["rlap_node_sample", "rlap_snapshot_plan_bytes", "rlap_edge_plan_build"]
    assert stub.exports()[-3][1]["p"] == [0.3, 0.45]
    b = stub.exports()[-1][1]
    assert (b["m"], b["S"], b["G"], b["n"], b["flags"], b["ptr"]) == (10, 2, 1, 6, 2 | 4 | 256, [0, 5, 10]) and plan.layers == 2


def test_layout_matches_the_header(tmp_path):
    """_lib.NodeSampleInfo and rlap_node_sample_info describe the same bytes (the check of tests/test_cabi_symbols.py's LAYOUTS)."""
    from rlap_amd import _lib
    cls, c_name = _lib.NodeSampleInfo, "rlap_node_sample_info"
    fields = [f for f, _ in cls._fields_]
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    end = hdr.index("} %s;" % c_name)
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    declared = [name for decl in re.findall(r"\b(?:int32_t|int64_t|float|double)\s+([a-z_0-9, ]+);", body) for name in decl.split(", ")]
    assert declared == fields == ["rows_needed", "launches", "arena_bytes", "host_syncs", "pad"]
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
    assert "rlap_node_sample" in _lib.EXPORTS and re.search(r"\bint rlap_node_sample\(rlap_handle h, const int64_t\* d_src", hdr)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rlap_node_sample")
    api = open(os.path.join(INC, "rlap_api.hip")).read()
    body = api[api.index("int rlap_node_sample("):api.index("int rlap_edge_drop(")]
    assert "poisoned_call(h," in body and "node_sample_run(" in body and "hipMalloc" not in body and "RLAP_E_TOO_LARGE" in body
    assert all(out in body[body.index("poisoned_call(h,"):] for out in ("d_rows", "d_ptr", "d_node_mask", "d_walks"))   # all four poisoned
    src = open(os.path.join(INC, "rlap_nodesample.hip")).read()
    assert "hipMalloc" not in src and src.count("hipStreamSynchronize(") == 1 and "asm" not in src   # scratch from the arena; one synchronisation
    assert not re.search(r"atomic\w*\([^;]*(double|float)", src)
    assert '#include "rlap_nodesample.h"' in src and '#include "rlap_nodesample.h"' in open(nodesample_mirror.SRC).read()   # one set of rules
    shared = open(os.path.join(INC, "rlap_rowcompact_dev.h")).read()                    # the compaction and the list builder: the same of them
    assert "hipMalloc" not in shared and "hipStreamSynchronize(" not in shared and "asm" not in shared
    assert not re.search(r"atomic\w*\([^;]*(double|float)", shared)
    assert '#include "rlap_rowcompact_dev.h"' in src and "struct Flip" not in src and not re.search(r"void k_\w+_(count|write)\b", src)
    assert "rowcompact" not in open(nodesample_mirror.SRC).read() and "rowcompact" not in open(os.path.join(INC, "rlap_nodesample.h")).read()
    mk = open(os.path.join(INC, "Makefile")).read()
    assert "rlap_nodesample.o" in mk and "rlap_nodesample.h" in mk and "-ffp-contract=off" in mk and "fast-math" not in mk
    import inspect
    from rlap_amd import ops
    assert '_device_call("rlap_node_sample"' in inspect.getsource(ops.sample_subgraphs)
