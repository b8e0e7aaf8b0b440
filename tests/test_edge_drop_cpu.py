"""Edge dropping without a GPU (rlap_edge_drop, ops.drop_edges).

1. The rules of rlap_amd/csrc/rlap_edgedrop.h -- compiled here with g++ through tests/csrc/edgedrop_mirror.cc, the same functions
   rlap_edgedrop.hip's kernels read -- against numpy restatements written from the prose of the rules alone: the three centralities,
   the coin (a pure-Python integer restatement, bit for bit), node_weight, the drop probability and the mask.  No coin of any case
   of tests/edge_drop_cases.py falls within BAND of its drop probability: the guarantee the GPU suite leans on.
2. The mirror as a stand-alone program under -fsanitize=address,undefined, malformed inputs included.
3. The Python -> C mapping of ops.drop_edges and the adapters on a stub library, every ValueError raised before the device is touched,
   the layout of rlap_edge_drop_info, and the export's place in the header, _lib.EXPORTS, the Makefile and the checked call path.

Measured (this file, recorded in DESIGN 4.20): PageRank against the sequential restatement at most 4.8e-15 relative (the comb, bound
1.1e-12) and 5.3e-16 on BA(300, 3) (bound 9.8e-14); eigenvector against eigh's Perron vector 1.3e-11 on BA(300, 3) after 45 steps
(bound 1.6e-9) and 3.1e-15 on the ring (bound 4.0e-8)."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import edge_drop_cases as cases
import edgedrop_mirror
from util import StubLib, f64_at, i64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
U = 2.0 ** -53
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return edgedrop_mirror.build(tmp_path_factory.mktemp("edgedrop"))


# ------------------------------------------------------------------------------------------------ restatements, from the prose
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def coin(seed, k, e):
    return (mix64(mix64(((seed + k) & M64) ^ 0x6564676564726F70) ^ mix64(e)) >> 11) * 2.0 ** -53


def np_mix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def np_coins(seed, K, E):
    with np.errstate(over="ignore"):
        rows = np_mix64(np.arange(E, dtype=np.uint64))
        return np.stack([(np_mix64(np.uint64(mix64(((seed + k) & M64) ^ 0x6564676564726F70)) ^ rows) >> np.uint64(11)).astype(np.float64) * U
                         for k in range(K)]).reshape(K, E)


def np_degree(src, dst, n):
    a, b = np.concatenate([src, dst]), np.concatenate([dst, src])
    pairs = np.unique(b * n + a)                       # distinct (u, v) of the symmetrised rows, keyed by v
    return np.bincount(pairs // n, minlength=n).astype(np.float64)


def np_pagerank(src, dst, n, damp, iters):
    out = np.bincount(src, minlength=n).astype(np.float64)
    x = np.ones(n)
    for _ in range(iters):
        agg = np.zeros(n)
        np.add.at(agg, dst, x[src] / out[src])
        x = (1.0 - damp) * x + damp * agg
    return x


def np_scores(c, cnt, E):
    """node_weight from a centrality and the counts, the sums exactly rounded (math.fsum)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.log(c)
        on = cnt > 0
        smax = s[on].max()
        smean = math.fsum((cnt[on] * s[on]).tolist()) / E
        w = (smax - s) / (smax - smean)
        wmean = math.fsum((cnt[on] * w[on]).tolist()) / E
        return w / wmean, s, smax, smean


def counts(src, dst, n, aggr):
    return np.bincount(src if aggr == "source" else dst, minlength=n)


# ------------------------------------------------------------------------------------------------ 1. the rules
def test_constants_and_key_bits(lib):
    assert lib.edgedrop_tile() == 256 and lib.edgedrop_row_tile() == cases.ROW_TILE and lib.edgedrop_max_views() == 32
    assert [lib.edgedrop_pair_key_bits(n) for n in (1, 2, 3, 1024, (1 << 31) - 1)] == [1, 2, 4, 20, 62]


@pytest.mark.parametrize("name", list(cases.GRAPHS))
def test_degree_equals_unique_pairs(lib, name):
    src, dst, n = cases.graph(name)
    got = edgedrop_mirror.run(lib, src, dst, n, scheme="degree")["centrality"]
    assert np.array_equal(got, np_degree(src, dst, n))
    if name in ("ba300", "ring64", "two_ba50", "comb"):                          # symmetric and coalesced: the in-degree
        assert np.array_equal(got, np.bincount(dst, minlength=n))
    if name == "directed":
        assert got.tolist() == [4.0, 3.0, 3.0, 3.0, 3.0, 3.0, 2.0, 0.0, 2.0]         # by hand: loops once, duplicates once, id 7 without rows


@pytest.mark.parametrize("name", list(cases.GRAPHS))
def test_pagerank_within_the_rounding_bound(lib, name):
    src, dst, n = cases.graph(name)
    for damp, iters in ((0.85, 10), (0.5, 3)):
        got = edgedrop_mirror.run(lib, src, dst, n, scheme="pagerank", pr_damp=damp, pr_iters=iters)
        want = np_pagerank(src, dst, n, damp, iters)
        dmax = int(np.bincount(dst, minlength=n).max())
        bound = 2 * iters * (dmax + 4) * U
        rel = np.abs(got["centrality"] - want) / want
        print(f"{name} damp {damp} iters {iters}: max relative difference {rel.max():.3e}, bound {bound:.3e}")
        assert got["iters"] == iters and (want > 0).all() and rel.max() <= bound


@pytest.mark.parametrize("name", cases.CONNECTED)
def test_eigenvector_against_the_perron_vector(lib, name):
    src, dst, n = cases.graph(name)
    tol = 1e-12
    got = edgedrop_mirror.run(lib, src, dst, n, scheme="eigenvector", evc_tol=tol, evc_max_iter=20000)
    A = np.zeros((n, n))
    np.add.at(A, (dst, src), 1.0)
    assert np.array_equal(A, A.T)
    lam, vec = np.linalg.eigh(A)
    perron = np.abs(vec[:, -1])
    rho = (lam[-2] + 1.0) / (lam[-1] + 1.0)
    bound = 2 * n * tol / (1.0 - rho) + 64 * n * U
    diff = np.abs((got["centrality"] - 1e-8) - perron).max()
    print(f"{name}: {got['iters']} steps, max difference to the Perron vector {diff:.3e}, bound {bound:.3e}, rho {rho:.6f}")
    assert got["converged"] and diff <= bound


def test_eigenvector_report_and_the_cut(lib):
    src, dst, n = cases.graph("ba300")
    cut = edgedrop_mirror.run(lib, src, dst, n, scheme="eigenvector", evc_tol=1e-12, evc_max_iter=3)
    assert (cut["iters"], cut["converged"]) == (3, False)
    full = edgedrop_mirror.run(lib, src, dst, n, scheme="eigenvector")
    assert full["converged"] and 3 < full["iters"] < 1000
    # a step by hand on the directed list: y = x + sum of x over the incoming rows (duplicates count), then y / ||y||_2
    src, dst, n = cases.graph("directed")
    one = edgedrop_mirror.run(lib, src, dst, n, scheme="eigenvector", evc_max_iter=1)
    y = (1.0 + np.bincount(dst, minlength=n)) / 3.0
    assert np.allclose(one["centrality"], y / np.sqrt((y * y).sum()) + 1e-8, rtol=8 * U, atol=0.0)


def test_coins_bit_for_bit(lib):
    for seed, k, e in [(0, 0, 0), (0, 1, 0), (20, 0, 1), (20, 31, 12345), (2**64 - 1, 1, 2**31 - 3), (2**63 + 5, 7, 2048), (7, 3, 2047)]:
        assert lib.edgedrop_coin(seed, k, e) == coin(seed, k, e)
    u = np_coins(cases.SEED, 2, 600)
    assert all(u[k, e] == coin(cases.SEED, k, e) == lib.edgedrop_coin(cases.SEED, k, e) for k in range(2) for e in range(0, 600, 7))
    assert 0.0 <= u.min() and u.max() < 1.0 and abs(u.mean() - 0.5) < 0.05


@pytest.mark.parametrize("name,scheme,aggr", cases.scored_cases())
def test_scores_probabilities_and_mask(lib, name, scheme, aggr):
    src, dst, n = cases.graph(name)
    E, K = src.size, len(cases.PS)
    w = cases.weights(E)
    got = edgedrop_mirror.run(lib, src, dst, n, w=w, p=cases.PS, scheme=scheme, threshold=cases.THRESHOLD, seed=cases.SEED, aggr=aggr)
    u = np_coins(cases.SEED, K, E)
    assert np.array_equal(got["u"], u)
    end = src if aggr == "source" else dst
    if scheme == "uniform":
        q = np.repeat(np.array(cases.PS)[:, None], E, 1)
        tol = np.zeros_like(q)
        assert not got["centrality"].any() and not got["node_weight"].any()
    else:
        cnt = counts(src, dst, n, aggr)
        nw, s, smax, smean = np_scores(got["centrality"], cnt, E)
        on = cnt > 0
        if name == "ring64":
            assert smax == smean and np.isnan(got["node_weight"]).all()
            tol_n = np.zeros(n)
        else:
            # the mirror's tree sums against exactly rounded ones: each of smean and wmean is off by at most N u times the mean
            # magnitude of its terms, so w by w N u max|s| / (smax - smean), and node_weight by twice that plus N u, relatively
            smag = np.abs(s[on]).max()
            tol_n = (1.0 + np.abs(nw)) * 4 * n * U * (1.0 + smag) / (smax - smean)
            assert smax > smean and np.all(np.abs(got["node_weight"][on] - nw[on]) <= tol_n[on])
            assert abs(math.fsum((cnt[on] * got["node_weight"][on]).tolist()) / E - 1.0) <= 4 * n * U   # mean weight of the rows: 1
        with np.errstate(invalid="ignore"):
            t = nw[end][None, :] * np.array(cases.PS)[:, None]
            q = np.where(t < cases.THRESHOLD, t, cases.THRESHOLD)
        tol = np.repeat(tol_n[end][None, :], K, 0)
    assert np.all(np.abs(got["q"] - q) <= tol) and (got["q"] <= max(cases.THRESHOLD, max(cases.PS))).all()
    band = np.abs(u - got["q"]) <= cases.BAND
    assert not band.any(), f"{int(band.sum())} rows inside the band: choose other seeds"
    assert np.array_equal(got["mask"], u >= q)
    # rows: the input rows at the mask's positions, in order, view-major; the weights untouched
    want = np.concatenate([np.stack([src[m], dst[m], w[m]], 1) for m in got["mask"]])
    assert np.array_equal(got["rows"], want) and got["ptr"].tolist() == [0] + np.cumsum(got["mask"].sum(1)).tolist()
    if name == "ring64":
        assert (got["q"] == (cases.THRESHOLD if scheme != "uniform" else q)).all()


def test_edge_cases(lib):
    src, dst, n = cases.graph("ba300")
    E = src.size
    for scheme in cases.SCHEMES:
        keep = edgedrop_mirror.run(lib, src, dst, n, p=[0.0, 0.0], scheme=scheme, seed=3)
        assert keep["mask"].all() and keep["ptr"].tolist() == [0, E, 2 * E] and np.array_equal(keep["rows"][:E, 0], src)
        assert (keep["rows"][:, 2] == 1.0).all()                                    # no weights given: 1.0
    none = edgedrop_mirror.run(lib, src, dst, n, p=[1.0, 0.0, 1.0], scheme="uniform")
    assert not none["mask"][0].any() and none["mask"][1].all() and none["ptr"].tolist() == [0, 0, E, E]   # empty views: equal offsets
    # view k of a K-view call is the one-view call with (p[k], seed + k)
    many = edgedrop_mirror.run(lib, src, dst, n, p=[0.2, 0.5, 0.35], scheme="pagerank", seed=40)
    for k, p in enumerate([0.2, 0.5, 0.35]):
        one = edgedrop_mirror.run(lib, src, dst, n, p=p, scheme="pagerank", seed=40 + k)
        assert np.array_equal(one["mask"][0], many["mask"][k]) and np.array_equal(one["rows"], many["rows"][many["ptr"][k]:many["ptr"][k + 1]])
    for E in cases.TILE_EDGE_ROWS:
        s, d, nn = cases.random_rows(E)
        for K in (1, 2, 3):
            got = edgedrop_mirror.run(lib, s, d, nn, p=[0.5] * K, scheme="uniform", seed=cases.SEED)
            assert got["mask"].shape == (K, E) and np.array_equal(got["mask"], np_coins(cases.SEED, K, E) >= 0.5)
            assert not (np.abs(got["u"] - 0.5) <= cases.BAND).any()
    for kw, status in [(dict(p=[0.5] * 33), 9), (dict(p=1.5), 3), (dict(p=-0.1), 3), (dict(threshold=1.5), 3),
                       (dict(scheme="pagerank", pr_damp=1.5), 3), (dict(scheme="eigenvector", evc_max_iter=0), 3)]:
        with pytest.raises(edgedrop_mirror.Refused) as e:
            edgedrop_mirror.run(lib, src, dst, n, **kw)
        assert e.value.status == status
    with pytest.raises(edgedrop_mirror.Refused) as e:
        edgedrop_mirror.run(lib, src, dst, n - 1)
    assert e.value.status == 2


def assert_no_coin_in_the_band(got, what):
    gap = float(np.abs(got["u"] - got["q"]).min())
    print(f"{what}: the smallest |u - q| is {gap:.2e}")
    assert gap > cases.BAND, f"{what}: a coin inside the band: choose another seed"
    return gap


def test_the_stride_constant_and_the_large_input(lib):
    """MAX_GRID_ROWS is what one round of a strided launch of rlap_edgedrop.hip covers; the large input of
    tests/test_gpu_augment_strides.py is one round, one whole wave and one lane."""
    src = open(os.path.join(INC, "rlap_edgedrop.hip")).read()
    grid = int(re.search(r"constexpr int64_t ED_MAX_GRID = (\d+);", src).group(1))
    assert "return capped_blocks(n, TILE, ED_MAX_GRID);" in src and cases.NODE_TILE == lib.edgedrop_tile()
    assert cases.MAX_GRID_ROWS == grid * lib.edgedrop_tile()
    assert cases.STRIDE_E == cases.MAX_GRID_ROWS + 64 + 1 and cases.STRIDE_N > cases.MAX_GRID_ROWS
    s, d, n = cases.stride_rows()
    assert s.size == d.size == cases.STRIDE_E and n == cases.STRIDE_N and 0 <= min(s.min(), d.min()) and max(s.max(), d.max()) < n


@pytest.mark.parametrize("scheme", cases.SCHEMES)
def test_no_coin_of_the_large_input_in_the_band(lib, scheme):
    s, d, n = cases.stride_rows()
    got = edgedrop_mirror.run(lib, s, d, n, w=cases.weights(s.size), p=cases.PS, scheme=scheme, threshold=cases.THRESHOLD, seed=cases.SEED,
                              aggr="sink", **cases.STRIDE_ITERS)
    assert_no_coin_in_the_band(got, f"large input, {scheme}")
    assert np.array_equal(got["mask"], got["u"] >= got["q"])
    if scheme != "uniform":
        on = np.bincount(d, minlength=n) > 0
        assert np.isfinite(got["node_weight"][on]).all() and on.sum() < n            # ids without incoming rows occur too


@pytest.mark.parametrize("n", cases.NODE_EDGE_NODES)
def test_node_tile_and_key_width_edges(lib, n):
    """The inputs of tests/test_gpu_edge_drop_regimes.py: the tiles of wg_total's stride, the key widths on both sides of a power of
    two, the top id at both ends, and no coin of any of the forty cases within BAND of its drop probability."""
    src, dst, nn = cases.node_edge_rows(n)
    assert nn == n and src.size == 3 * n + 7 and (src[:3] == n - 1).all() and (dst[1:5] == n - 1).all() and max(src.max(), dst.max()) == n - 1
    tiles = -(-n // cases.NODE_TILE)
    assert tiles == {255: 1, 256: 1, 257: 2, 65536: 256, 65537: 257}[n]
    strides = -(-tiles // cases.NODE_TILE)                                           # the trips of lane 0 through wg_total's loop
    assert strides == (2 if n == 65537 else 1)
    assert lib.edgedrop_pair_key_bits(n) == {255: 16, 256: 16, 257: 17, 65536: 32, 65537: 33}[n]
    w = cases.weights(src.size)
    for scheme in cases.SCHEMES:
        for aggr in ("sink", "source"):
            got = edgedrop_mirror.run(lib, src, dst, n, w=w, p=cases.PS, scheme=scheme, threshold=cases.THRESHOLD, seed=cases.SEED, aggr=aggr,
                                      **cases.NODE_EDGE_ITERS)
            assert_no_coin_in_the_band(got, f"n = {n}, {scheme}, {aggr}")
            assert np.array_equal(got["u"], np_coins(cases.SEED, len(cases.PS), src.size))
            if scheme == "degree":
                assert np.array_equal(got["centrality"], np_degree(src, dst, n))
            if scheme == "eigenvector":
                assert (got["iters"], got["converged"]) == (cases.NODE_EDGE_ITERS["evc_max_iter"], False)


@pytest.mark.parametrize("variant", list(cases.RUN_VARIANTS))
def test_sorted_rows_and_their_runs(lib, variant):
    """Where the runs of the sorted row lists fall in the waves (64 lanes) and workgroups (256 rows) of the keys kernel, asserted
    from the positions; and the bands of the cases the GPU suite runs on them."""
    front, by_source = cases.RUN_VARIANTS[variant]
    src, dst, n = cases.runs(front, by_source)
    ids = src if by_source else dst
    assert ids.size == sum(cases.RUN_DEGREES) + front and (np.diff(ids[front:]) >= 0).all()
    spans = cases.run_spans(ids)
    assert [b - a + 1 for a, b in spans[front:]] == list(cases.RUN_DEGREES)
    facts = dict(starts_on_lane_0=any(a % 64 == 0 and b > a for a, b in spans), ends_on_lane_63=any(b % 64 == 63 and b > a for a, b in spans),
                 whole_wave=any(a % 64 == 0 and b - a + 1 == 64 for a, b in spans), covers_waves=any(b // 64 - a // 64 >= 2 for a, b in spans),
                 crosses_row_256=any(a < 256 <= b for a, b in spans), partial_last_wave=ids.size % 64 != 0)
    if front:                                                                        # every run one lane on: none starts on lane 0
        assert facts == dict(starts_on_lane_0=False, ends_on_lane_63=False, whole_wave=False, covers_waves=True, crosses_row_256=True,
                             partial_last_wave=True)
        assert any(a % 64 == 1 and b % 64 == 0 for a, b in spans)                    # the run of 64: lane 1 to lane 0 of the next wave
    else:
        assert all(facts.values())
    w = cases.weights(src.size)
    for scheme in ("pagerank", "degree"):
        for aggr in ("sink", "source"):
            got = edgedrop_mirror.run(lib, src, dst, n, w=w, p=cases.PS, scheme=scheme, threshold=cases.THRESHOLD, seed=cases.SEED, aggr=aggr)
            assert_no_coin_in_the_band(got, f"runs {variant}, {scheme}, {aggr}")
            cnt = counts(src, dst, n, aggr)
            assert np.isfinite(got["node_weight"][cnt > 0]).all()                    # smax > smean: the scores are not degenerate
            if scheme == "degree":
                assert np.array_equal(got["centrality"], np_degree(src, dst, n))


@pytest.mark.parametrize("scheme", ("uniform", "degree"))
def test_thirty_two_views(lib, scheme):
    src, dst, n = cases.random_rows(cases.ROW_TILE + 1)
    got = edgedrop_mirror.run(lib, src, dst, n, p=cases.MANY_PS, scheme=scheme, threshold=cases.THRESHOLD, seed=cases.SEED)
    assert len(cases.MANY_PS) == lib.edgedrop_max_views() and got["mask"].shape == (32, cases.ROW_TILE + 1)
    assert_no_coin_in_the_band(got, f"32 views, {scheme}")
    assert got["mask"][0].all() and 0 < got["mask"][31].sum() < src.size
    for k in (0, 31):
        one = edgedrop_mirror.run(lib, src, dst, n, p=cases.MANY_PS[k], scheme=scheme, threshold=cases.THRESHOLD, seed=cases.SEED + k)
        assert np.array_equal(one["mask"][0], got["mask"][k])


# ------------------------------------------------------------------------------------------------ 2. the sanitizer program
def test_the_mirror_under_asan_and_ubsan(tmp_path):
    """The mirror as a stand-alone program with its own main: a plain executable, nothing preloaded.  Its last inputs are malformed
    (ids out of range, 33 views, p = 1.5, an unknown scheme): it reports the refusals and exits clean."""
    exe = tmp_path / "edgedrop_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", INC, "-o", str(exe), edgedrop_mirror.MAIN])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": ok (") == 3 * 4 * 2 + 6 * 3 + 3 and "FAILED" not in r.stdout and "0 failures" in r.stdout
    assert r.stdout.count("refused as expected") == 10


# ------------------------------------------------------------------------------------------------ 3. the entry points
SIGS = {
    "rlap_edge_drop": "h src dst w E n scheme flags p K threshold seed damp pr_iters evc_tol evc_max_iter rows cap ptr mask centrality node_weight info",
    "rlap_snapshot_plan_bytes": "m S G n flags bytes",
    "rlap_edge_plan_build": "h sc m ptr S node_ptr G n flags fill plan plan_bytes desc info",
}
ARENA = 555


class DropStub(StubLib):
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
        rec = {k: a[k] for k in ("E", "n", "scheme", "flags", "K", "threshold", "seed", "damp", "pr_iters", "evc_tol", "evc_max_iter", "cap")}
        rec["p"] = list(a["p"])
        rec["src"] = i64_at(a["src"], E) if E else a["src"]
        rec["dst"] = i64_at(a["dst"], E) if E else a["dst"]
        rec["w"] = None if a["w"] is None else f64_at(a["w"], E)
        rec["has"] = tuple(a[k] is not None for k in ("mask", "centrality", "node_weight"))
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
        if a["mask"]:
            ctypes.memset(a["mask"], 1, K * E)
        info = a["info"]._obj
        info.rows_needed, info.arena_bytes, info.iters, info.converged, info.host_syncs = K * E, ARENA, 17, 1, 1
        return 0


@pytest.fixture
def stub(monkeypatch):
    return stub_ops(monkeypatch, DropStub())


EI = torch.tensor([[2, 0, 2, 0, 3], [0, 1, 2, 1, 2]])


def test_drop_edges_arguments(stub):
    from rlap_amd import ops
    rows, ptr = ops.drop_edges(EI)
    (name, b), = stub.exports()
    assert name == "rlap_edge_drop" and (b["E"], b["n"], b["scheme"], b["flags"], b["K"], b["p"]) == (5, 4, 0, 0, 1, [0.5])      # max id + 1
    assert (b["threshold"], b["seed"], b["damp"], b["pr_iters"], b["evc_tol"], b["evc_max_iter"], b["cap"]) == (0.7, 0, 0.85, 10, 1e-6, 1000, 5)
    assert b["src"] == [2, 0, 2, 0, 3] and b["dst"] == [0, 1, 2, 1, 2] and b["w"] is None and b["has"] == (False, False, False)
    assert rows.dtype == torch.float64 and rows.tolist() == [[2, 0, 1], [0, 1, 1], [2, 2, 1], [0, 1, 1], [3, 2, 1]] and ptr.tolist() == [0, 5]
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["arena_bytes"] == ARENA and ops.last_stats["rows_needed"] == 5
    w = torch.tensor([0.5, 0.25, 2.0, 4.0, 1.5], dtype=torch.float32)
    out = ops.drop_edges(EI.int(), w, 9, [0.1, 0.2, 0.3], "eigenvector", 0.6, -1, "source", 0.5, 4, 1e-3, 77, return_mask=True, return_scores=True)
    b = stub.exports()[-1][1]
    assert (b["n"], b["scheme"], b["flags"], b["K"], b["p"], b["threshold"], b["seed"]) == (9, 3, 1, 3, [0.1, 0.2, 0.3], 0.6, 2**64 - 1)
    assert (b["damp"], b["pr_iters"], b["evc_tol"], b["evc_max_iter"], b["cap"], b["has"]) == (0.5, 4, 1e-3, 77, 15, (True, True, True))
    assert b["w"] == [0.5, 0.25, 2.0, 4.0, 1.5]
    rows, ptr, mask, scores = out
    assert tuple(rows.shape) == (15, 3) and ptr.tolist() == [0, 5, 10, 15] and mask.dtype == torch.bool and tuple(mask.shape) == (3, 5) and mask.all()
    assert rows[5:10, 2].tolist() == [0.5, 0.25, 2.0, 4.0, 1.5]
    assert set(scores) == {"centrality", "node_weight", "iters", "converged"} and scores["iters"] == 17 and scores["converged"] is True
    assert tuple(scores["centrality"].shape) == (9,) and scores["node_weight"].dtype == torch.float64
    for scheme, code in (("uniform", 0), ("degree", 1), ("pagerank", 2), ("eigenvector", 3)):
        ops.drop_edges(EI, scheme=scheme, p=(0.25,))
        assert stub.exports()[-1][1]["scheme"] == code
    rows, ptr = ops.drop_edges(torch.zeros((2, 0), dtype=torch.int64), p=[0.5, 0.5])
    b = stub.exports()[-1][1]
    assert (b["E"], b["n"], b["src"], b["cap"]) == (0, 0, None, 0) and tuple(rows.shape) == (0, 3) and ptr.tolist() == [0, 0, 0]


def test_host_checks_launch_nothing(stub):
    from rlap_amd import ops
    for args, kw, msg in [((EI.double(),), {}, "edge_index"), ((EI[0],), {}, "edge_index"), ((torch.zeros((3, 2), dtype=torch.int64),), {}, "edge_index"),
                          ((EI, torch.ones(3)), {}, "edge_weight"), ((EI, torch.ones(5, dtype=torch.int64)), {}, "edge_weight"),
                          ((EI,), dict(num_nodes=-2), "num_nodes"), ((EI,), dict(num_nodes=2.5), "num_nodes"),
                          ((EI,), dict(p=1.5), "p:"), ((EI,), dict(p=[0.5, -0.1]), "p:"), ((EI,), dict(p=[0.5] * 33), "p:"), ((EI,), dict(p=[]), "p:"),
                          ((EI,), dict(p="0.5"), "p:"), ((EI,), dict(p=float("nan")), "p:"), ((EI,), dict(p=True), "p:"), ((EI,), dict(p=None), "p:"),
                          ((EI,), dict(p=np.array([0.5, 1.5])), "p:"), ((EI,), dict(p=torch.ones(2, 2)), "p:"), ((EI,), dict(p=np.zeros(33)), "p:"),
                          ((EI,), dict(scheme="katz"), "scheme"), ((EI,), dict(scheme=None), "scheme"),
                          ((EI,), dict(aggr="mean"), "aggr"), ((EI,), dict(threshold=1.2), "threshold"), ((EI,), dict(threshold=None), "threshold"),
                          ((EI,), dict(seed=1.5), "seed"), ((EI,), dict(seed="7"), "seed"), ((EI,), dict(pr_damp=-0.1), "pr_damp"), ((EI,), dict(pr_iters=-1), "pr_iters"),
                          ((EI,), dict(pr_iters=2.0), "pr_iters"), ((EI,), dict(evc_tol=-1e-6), "evc_tol"), ((EI,), dict(evc_tol=float("inf")), "evc_tol"),
                          ((EI,), dict(evc_max_iter=0), "evc_max_iter"), ((EI,), dict(evc_max_iter=10**6), "evc_max_iter")]:
        with pytest.raises(ValueError, match=msg):
            ops.drop_edges(*args, **kw)
    assert stub.exports() == [] and ops.last_stats is None


@pytest.mark.parametrize("status,error,text", [(2, ValueError, "status 2"), (3, ValueError, "status 3"), (9, RuntimeError, "status 9"),
                                               (13, RuntimeError, "status 13")])
def test_device_statuses(stub, status, error, text):
    from rlap_amd import ops
    stub.status = status
    with pytest.raises(error, match=text):
        ops.drop_edges(EI, scheme="degree")
    assert ops.last_stats is None and [c[0] for c in stub.exports()] == ["rlap_edge_drop"]


def test_p_takes_any_number_and_any_sequence(stub):
    from rlap_amd import ops
    for p, want in [(np.float32(0.25), [0.25]), (torch.tensor(0.25), [0.25]), (np.array(0.5), [0.5]), (1, [1.0]), (np.array([0.25, 0.5]), [0.25, 0.5]),
                    (torch.tensor([0.25, 0.5, 0.75]), [0.25, 0.5, 0.75]), ((np.float32(0.5), 0), [0.5, 0.0]), (iter([0.5]), [0.5])]:
        ops.drop_edges(EI, p=p)
        assert stub.exports()[-1][1]["p"] == want
    ops.drop_edges(EI, threshold=np.float64(0.5), pr_damp=torch.tensor(0.5))
    assert (stub.exports()[-1][1]["threshold"], stub.exports()[-1][1]["damp"]) == (0.5, 0.5)


def test_seeds_none_draws_per_call_an_integer_repeats(stub):
    """The reference builds aug1 and aug2 with the same arguments and calls them every step: default-constructed augmentors draw a
    fresh seed per call (torch's RNG, as adapters.rLap), so neither two augmentors nor two calls of one share their coins; an
    explicit seed is passed on as it is."""
    from rlap_amd import adapters, ops
    x = torch.ones(4, 3)
    seeds = lambda: [c[1]["seed"] for c in stub.exports() if c[0] == "rlap_edge_drop"]
    for cls in (adapters.EdgeDropping, adapters.EdgeDroppingDegree, adapters.EdgeDroppingPR, adapters.EdgeDroppingEVC):
        stub.calls.clear()
        aug1, aug2 = (cls(0.3), cls(0.3)) if cls is adapters.EdgeDropping else (cls(0.3, 0.7), cls(0.3, 0.7))
        aug1(x, EI), aug2(x, EI), aug1(x, EI), aug2.augment((x, EI, None))
        assert len(set(seeds())) == 4 and aug1.last_seed == seeds()[2] and aug2.last_seed == seeds()[3]
        fixed = cls(0.3, seed=11) if cls is adapters.EdgeDropping else cls(0.3, 0.7, 11)
        fixed(x, EI), fixed(x, EI)
        assert seeds()[-2:] == [11, 11] and fixed.last_seed == 11
    stub.calls.clear()
    views = adapters.EdgeDroppingViews("degree", (0.3, 0.3), 0.7)
    for _ in range(2):                                                              # two steps of the (aug1, aug2) pair: one call a step
        for aug in views.augmentors():
            aug(x, EI)
    views.augment((x, EI, None)), views.plan((x, EI, None))
    assert len(seeds()) == 4 and len(set(seeds())) == 4 and views.last_seed == seeds()[-1]
    assert all(abs(a - b) > 1 for a in seeds() for b in seeds() if a != b)           # view k uses seed + k: no view shares another call's coins
    fixed = adapters.EdgeDroppingViews("degree", (0.3, 0.3), 0.7, 5)
    fixed.augment((x, EI, None)), fixed.augment((x, EI, None))
    assert seeds()[-2:] == [5, 5]
    torch.manual_seed(3)
    ops.drop_edges(EI, seed=None)
    first = seeds()[-1]
    ops.drop_edges(EI, seed=None)
    torch.manual_seed(3)
    ops.drop_edges(EI, seed=None)
    assert seeds()[-2] != first and seeds()[-1] == first and 0 <= first < 2**62      # from torch's RNG: reproducible under manual_seed
    with pytest.raises(ValueError, match="ps"):
        adapters.EdgeDroppingViews("degree", ())


def test_adapters_reach_the_call(stub):
    from rlap_amd import adapters
    x = torch.ones(6, 3, dtype=torch.float64)
    w = torch.tensor([0.5, 0.25, 2.0, 4.0, 1.5], dtype=torch.float64)
    for cls, code in ((adapters.EdgeDropping, 0), (adapters.EdgeDroppingDegree, 1), (adapters.EdgeDroppingPR, 2), (adapters.EdgeDroppingEVC, 3)):
        aug = cls(0.3) if code == 0 else cls(0.3, 0.6)
        g = aug(x, EI, w)
        b = stub.exports()[-1][1]
        assert (b["scheme"], b["p"], b["threshold"], b["flags"], b["n"]) == (code, [0.3], 1.0 if code == 0 else 0.6, 0, 4)   # max id + 1, as the reference
        assert g.x is x and g.edge_index.dtype == torch.int64 and torch.equal(g.edge_index, EI) and torch.equal(g.edge_weights, w)
        g = aug.augment((x, EI, None))
        assert g.edge_weights is None and torch.equal(g.edge_index, EI)
    views = adapters.EdgeDroppingViews("pagerank", (0.3, 0.45), 0.7, 5)
    graphs = views.augment(adapters.Graph(x, EI, w))
    b = stub.exports()[-1][1]
    assert (b["scheme"], b["p"], b["seed"], b["K"], b["n"]) == (2, [0.3, 0.45], 5, 2, 6) and len(graphs) == 2 and torch.equal(graphs[1].edge_index, EI)
    before = len(stub.exports())
    aug1, aug2 = views.augmentors()
    g1, g2 = aug1(x, EI, w), aug2(x, EI, w)
    assert len(stub.exports()) == before + 1 and torch.equal(g1.edge_weights, w) and torch.equal(g2.edge_index, EI)   # the pair shares one call
    aug1(x, EI, w)
    assert len(stub.exports()) == before + 2
    plan = views.plan(adapters.Graph(x, EI, None), directions="forward")
    names = [c[0] for c in stub.exports()[-3:]]
    b = stub.exports()[-1][1]
    assert names == ["rlap_edge_drop", "rlap_snapshot_plan_bytes", "rlap_edge_plan_build"]
    assert (b["m"], b["S"], b["G"], b["n"], b["flags"], b["ptr"]) == (10, 2, 1, 6, 2 | 4 | 256, [0, 5, 10]) and plan.layers == 2


def test_layout_matches_the_header(tmp_path):
    """_lib.EdgeDropInfo and rlap_edge_drop_info describe the same bytes (the check of tests/test_cabi_symbols.py's LAYOUTS)."""
    from rlap_amd import _lib
    cls, c_name = _lib.EdgeDropInfo, "rlap_edge_drop_info"
    fields = [f for f, _ in cls._fields_]
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    end = hdr.index("} %s;" % c_name)
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    declared = [name for decl in re.findall(r"\b(?:int32_t|int64_t|float|double)\s+([a-z_0-9, ]+);", body) for name in decl.split(", ")]
    assert declared == fields
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
    assert "rlap_edge_drop" in _lib.EXPORTS and re.search(r"\bint rlap_edge_drop\(rlap_handle h, const int64_t\* d_src", hdr)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "rlap_edge_drop")
    api = open(os.path.join(INC, "rlap_api.hip")).read()
    body = api[api.index("int rlap_edge_drop("):api.index("int rlap_snapshot_plan_propagate(")]
    assert "poisoned_call(h," in body and "edge_drop_run(" in body and "hipMalloc" not in body and "RLAP_E_TOO_LARGE" in body
    assert all(out in body[body.index("poisoned_call(h,"):] for out in ("d_rows", "d_ptr", "d_mask", "d_centrality", "d_node_weight"))   # all five poisoned
    src = open(os.path.join(INC, "rlap_edgedrop.hip")).read()
    assert "hipMalloc" not in src and src.count("hipStreamSynchronize(") == 1 and "asm" not in src   # scratch from the arena; one synchronisation
    assert not re.search(r"atomic\w*\([^;]*(double|float)", src)
    shared = open(os.path.join(INC, "rlap_rowcompact_dev.h")).read()                    # the compaction and the list builder: the same of them
    assert "hipMalloc" not in shared and "hipStreamSynchronize(" not in shared and "asm" not in shared
    assert not re.search(r"atomic\w*\([^;]*(double|float)", shared)
    assert '#include "rlap_rowcompact_dev.h"' in src and "struct Flip" not in src and not re.search(r"void k_\w+_(count|write)\b", src)
    mk = open(os.path.join(INC, "Makefile")).read()
    assert "rlap_edgedrop.o" in mk and "rlap_edgedrop.h" in mk and "-ffp-contract=off" in mk and "fast-math" not in mk
    assert "rlap_rowcompact_dev.h" in mk
    import inspect
    from rlap_amd import ops
    assert '_device_call("rlap_edge_drop"' in inspect.getsource(ops.drop_edges)
