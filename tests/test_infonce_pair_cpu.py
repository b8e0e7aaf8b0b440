"""The symmetric InfoNCE pair (ops.info_nce_pair, rlap_infonce_pair / rlap_infonce_pair_backward) without a GPU:

  * the rule -- the pair's host mirror (tests/csrc/infonce_pair_mirror.cc, every value from rlap_amd/csrc/rlap_infonce.h, contraction
    off) against the float64 restatement 0.5 * (l(a, b) + l(b, a)) and against two runs of the one-direction mirror, for both
    `positive` settings and tau in {1/32, 0.4, 2}; the work split and the column-sum order; the invariances;
  * the index arithmetic of the split in a stand-alone program under -fsanitize=address,undefined, exhaustively for N <= 300;
  * the Python -> C mapping of both exports on a stub library, the layout of rlap_infonce_pair_info, adapters.NodeContrast(pair=True).

The bounds are four times the largest differences measured with these inputs (DESIGN 4.19 has the figures), as in
tests/test_infonce_cpu.py.  Measured here, pair mirror against the restatement: loss 2.01e-7 relative, gradients 1.68e-6 of the
largest entry.  Pair mirror against two runs of the one-direction mirror: s_ii bit for bit; gradients 1.05e-6 of the largest entry
(one float32 chain of e (1/Z_i + 1/Zc_j) against the float64 sum of two float32 chains); the loss differed in NO bit at these shapes,
so its bound is not four times a measurement but the float64 arithmetic's: the two differ only in the order of the float64 sums that
make Z and Zc (N non-negative terms: at most N 2^-53 relative each way, so log Z moves by at most N 2^-52) and in the last place of
a row term and of the chunk sums (|row| < 64: 2^-46 each) -- PAIR_LOSS_ABS(N) = (N + 256) 2^-52, absolute.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import infonce_mirror as im
import infonce_pair_mirror as pm
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, f64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_BOUND = 4 * 2.01e-7          # against the restatement, relative to the loss
GRAD_BOUND = 4 * 1.68e-6          # against the restatement, relative to the largest gradient entry
PAIR_GRAD_BOUND = 4 * 1.05e-6     # against two runs of the one-direction mirror, relative to the largest gradient entry


def pair_loss_abs(n):
    return (n + 256) * 2.0 ** -52


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return pm.build(tmp_path_factory.mktemp("infonce_pair"))


@pytest.fixture(scope="module")
def mirror1(tmp_path_factory):
    return im.build(tmp_path_factory.mktemp("infonce_one"))


def views(n, f, seed):
    """Two float32 views whose positives have cosine about 0.3."""
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((n, f)).astype(np.float32)
    b = (0.3 * a + rng.standard_normal((n, f))).astype(np.float32)
    return a, b


# ------------------------------------------------------------------------------------------------ the rule
SHAPES = [(33, 3), (65, 33), (300, 100), (129, 512)]
RULE = [(n, f, positive, tau) for n, f in SHAPES for positive in ("scaled", "raw") for tau in (1.0 / 32.0, 0.4, 2.0)]
G_UP = 0.75


@pytest.fixture(scope="module")
def pair_runs(mirror):
    cache = {}

    def get(n, f, positive, tau):
        key = (n, f, positive, tau)
        if key not in cache:
            a, b = views(n, f, 1000 + n)
            cache[key] = (a, b, pm.run(mirror, a, b, tau, positive, g=G_UP))
        return cache[key]
    return get


@pytest.mark.parametrize("n,f,positive,tau", RULE)
def test_mirror_against_the_float64_restatement(pair_runs, n, f, positive, tau):
    a, b, m = pair_runs(n, f, positive, tau)
    loss, ga, gb = pm.restatement(a, b, tau, positive, g=G_UP)
    rel = abs(m["loss"] - loss) / abs(loss)
    gmax = max(np.abs(ga).max(), np.abs(gb).max())
    grel = max(np.abs(m["ga"] - ga).max(), np.abs(m["gb"] - gb).max()) / gmax
    print(f"n={n} F={f} {positive} tau={tau}: loss {loss:.6g} rel {rel:.3g}, gradients rel {grel:.3g}")
    assert 0.05 < abs(loss) < 50.0                                # the relative error is meaningful
    assert rel <= LOSS_BOUND
    assert grel <= GRAD_BOUND
    assert np.isfinite(m["rows"]).all() and abs(-m["rows"].mean() - loss) <= LOSS_BOUND * abs(loss)


@pytest.mark.parametrize("n,f,positive,tau", RULE)
def test_mirror_against_two_runs_of_the_one_direction_mirror(pair_runs, mirror1, n, f, positive, tau):
    a, b, m = pair_runs(n, f, positive, tau)
    t = pm.two_runs(mirror1, a, b, tau, positive, g=G_UP)
    assert m["sii"].tobytes() == t["sii"].tobytes() == t["sii_swapped"].tobytes()      # fmaf(x, y, acc) == fmaf(y, x, acc)
    gmax = max(np.abs(t["ga"]).max(), np.abs(t["gb"]).max())
    dl = abs(m["loss"] - t["loss"])
    grel = max(np.abs(m["ga"] - t["ga"]).max(), np.abs(m["gb"] - t["gb"]).max()) / gmax
    zrel = (np.abs(m["z"] - t["z"]) / t["z"]).max()
    print(f"n={n} F={f} {positive} tau={tau}: loss diff {dl:.3g}, gradients rel {grel:.3g}, Z and Zc rel {zrel:.3g}")
    assert dl <= pair_loss_abs(n)
    assert grel <= PAIR_GRAD_BOUND
    assert zrel <= n * 2.0 ** -52                                 # the same float64 terms in another order


def test_raw_and_scaled_differ_in_the_positive_term_alone(mirror):
    a, b = views(65, 33, 5)
    s = pm.run(mirror, a, b, 0.4, "scaled")
    r = pm.run(mirror, a, b, 0.4, "raw")
    assert s["z"].tobytes() == r["z"].tobytes() and s["sii"].tobytes() == r["sii"].tobytes()
    want = s["rows"] - (1.0 / 0.4 - 1.0) * s["sii"].astype(np.float64)[None, :]
    assert np.abs(r["rows"] - want).max() < 1e-12


def test_swapping_the_views_swaps_the_lists_up_to_the_order_of_the_sums(mirror):
    """Z of (b, a) is Zc of (a, b) in another order, and the other way round: a swap of the two reciprocals or of rows and columns in
    the mirror would show here, where Z and Zc differ by far more than a summation order."""
    a, b = views(65, 33, 5)
    b[:20] *= -1.0                                                # makes S far from symmetric
    m, w = pm.run(mirror, a, b, 0.4, "raw", g=1.0), pm.run(mirror, b, a, 0.4, "raw", g=1.0)
    assert (np.abs(m["z"][0] - m["z"][1]) / m["z"][0]).max() > 1e-3
    assert (np.abs(m["z"][0] - w["z"][1]) / m["z"][0]).max() <= 65 * 2.0 ** -52
    assert (np.abs(m["z"][1] - w["z"][0]) / m["z"][1]).max() <= 65 * 2.0 ** -52
    assert abs(m["loss"] - w["loss"]) <= pair_loss_abs(65)
    gmax = np.abs(m["ga"]).max()
    assert np.abs(m["ga"] - w["gb"]).max() <= PAIR_GRAD_BOUND * gmax and np.abs(m["gb"] - w["ga"]).max() <= PAIR_GRAD_BOUND * gmax


# ------------------------------------------------------------------------------------------------ the work split
SPLIT_NS = list(range(1, 301)) + [2708, 4133, 34493, 169343]


def test_groups_and_parts_depend_on_n_alone_and_cover_everything_once(mirror):
    for n in SPLIT_NS:
        tiles = (n + 31) // 32
        blocks = (tiles + 3) // 4
        g, p = mirror.pair_groups(n), mirror.pair_parts(n)
        assert 1 <= g <= min(blocks, 16) and 1 <= p <= min(tiles, 512), n
        gb = [mirror.pair_group_begin(n, k) for k in range(g + 1)]
        pb = [mirror.pair_part_begin(n, k) for k in range(p + 1)]
        assert gb[0] == 0 and gb[-1] == blocks and all(x < y for x, y in zip(gb, gb[1:])), n      # contiguous, none empty: every
        assert pb[0] == 0 and pb[-1] == tiles and all(x < y for x, y in zip(pb, pb[1:])), n       # block and tile exactly once
        assert max(y - x for x, y in zip(pb, pb[1:])) <= max(mirror.pair_span_tiles(n), 1) or mirror.pair_span_tiles(n) == mirror.pair_span_cap()
    assert (mirror.pair_groups(2708), mirror.pair_parts(2708)) == (16, 32)
    sizes = lambda n: sorted({mirror.pair_group_begin(n, k + 1) - mirror.pair_group_begin(n, k) for k in range(mirror.pair_groups(n))})
    assert sizes(2708) == [1, 2] and sizes(4133) == [2, 3]
    assert (mirror.pair_groups(169343), mirror.pair_parts(169343), mirror.pair_span_tiles(169343)) == (16, 32, 166)
    assert mirror.pair_parts(300) == 10 and mirror.pair_groups(300) == 3


def test_the_partial_arrays_stay_linear_in_n(mirror):
    """(parts + groups) x Np doubles, parts <= 512 and groups <= 16 whatever N: the one-direction call's num_parts is 1 for large N
    and could not serve (one column partial per row block would be N^2 / 128 doubles)."""
    for n in SPLIT_NS + [1 << 20, (1 << 31) - 1]:
        npad = 32 * ((n + 31) // 32)
        cells = (mirror.pair_parts(n) + mirror.pair_groups(n)) * npad
        assert cells <= (512 + 16) * npad
        assert mirror.pair_span_tiles(n) <= mirror.pair_span_cap() == 256         # the column array in LDS: at most 64 KB


def test_tree32_is_the_butterfly(mirror):
    """tree32 against the butterfly written out on 32 'lanes' in numpy: x = x + x[lane ^ m] for m = 1, 2, 4, 8, 16; every lane ends
    with the same bits."""
    rng = np.random.RandomState(3)
    for _ in range(50):
        x = np.exp(rng.uniform(-40, 0, 32))
        v = x.copy()
        for m in (1, 2, 4, 8, 16):
            v = v + v[np.arange(32) ^ m]
        assert len({e.tobytes() for e in v}) == 1
        got = mirror.pair_tree32(np.ascontiguousarray(x).ctypes.data)
        assert np.float64(got).tobytes() == v[0].tobytes()


@pytest.mark.parametrize("f,pad", [(3, 1), (31, 1), (32, 32), (33, 31)])
def test_zero_feature_columns_change_no_bit(mirror, f, pad):
    a, b = views(65, f, 11)
    wide = lambda x: np.concatenate([x, np.zeros((x.shape[0], pad), dtype=np.float32)], axis=1)
    m = pm.run(mirror, a, b, 0.4, "scaled", g=1.0)
    w = pm.run(mirror, wide(a), wide(b), 0.4, "scaled", g=1.0)
    for key in ("loss", "z", "rows"):
        assert np.asarray(m[key]).tobytes() == np.asarray(w[key]).tobytes(), key
    for key in ("ga", "gb"):
        assert m[key].tobytes() == w[key][:, :f].tobytes() and not w[key][:, f:].any(), key


def test_a_zero_row_gives_finite_values(mirror):
    a, b = views(40, 5, 13)
    a[3] = 0.0
    b[17] = 0.0
    m = pm.run(mirror, a, b, 0.4, "raw", g=1.0)
    for key in ("loss", "z", "rows", "ga", "gb"):
        assert np.isfinite(np.asarray(m[key])).all(), key
    assert m["sii"][3] == 0.0 and m["sii"][17] == 0.0
    loss, _, _ = pm.restatement(a, b, 0.4, "raw")
    assert abs(m["loss"] - loss) <= LOSS_BOUND * abs(loss)


# ------------------------------------------------------------------------------------------------ the index arithmetic, under the sanitizers
def test_the_index_arithmetic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "infonce_pair_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "infonce_pair_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "300 sizes, 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_infonce": "h a b n F tau flags loss rows z info",
    "rlap_infonce_backward": "h a b n F tau flags z g ga gb info",
    "rlap_infonce_pair": "h a b n F tau flags loss rows z info",
    "rlap_infonce_pair_backward": "h a b n F tau flags z g ga gb info",
}
ARENA = 9876


def f32_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


class PairStub(StubLib):
    """Records the four exports.  Forward: loss = 1.5, rows = -1, z = 2 (pair: the first list; the second list rows = -3, z = 5);
    backward: ga = 3, gb = 4."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        status = self.statuses.pop(0) if self.statuses else self.status
        n, F = a["n"], a["F"]
        pair = "pair" in name
        lists = 2 if pair else 1
        rec = {k: a[k] for k in ("n", "F", "tau", "flags")}
        rec["a"], rec["b"] = f32_at(a["a"], n * F), f32_at(a["b"], n * F)
        back = name.endswith("backward")
        if back:
            rec["z"], rec["g"] = f64_at(a["z"], lists * n), f64_at(a["g"], 1)
        self.calls.append((name, rec))
        if status:
            return status
        if back:
            for key, v in (("ga", 3.0), ("gb", 4.0)):
                out = ctypes.cast(a[key], ctypes.POINTER(ctypes.c_float))
                for i in range(n * F):
                    out[i] = v
        else:
            ctypes.cast(a["loss"], ctypes.POINTER(ctypes.c_double))[0] = 1.5
            assert a["rows"] == a["loss"] + 8 and a["z"] == a["loss"] + 8 * (1 + lists * n)    # one buffer: loss | rows | z
            for key, v, v2 in (("rows", -1.0, -3.0), ("z", 2.0, 5.0)):
                out = ctypes.cast(a[key], ctypes.POINTER(ctypes.c_double))
                for i in range(lists * n):
                    out[i] = v if i < n else v2
        info = a["info"]._obj
        info.rows, info.features, info.parts, info.arena_bytes, info.host_syncs = n, F, 7, ARENA, 0
        if pair:
            info.groups = 3
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, PairStub())


def feats(n, f, shift=0.0):
    return (torch.arange(n * f, dtype=torch.float32).reshape(n, f) / 4.0 - 1.0 + shift)


@pytest.mark.parametrize("positive,flags", [("scaled", 0), ("raw", 1)])
def test_arguments_of_the_forward_export(lib, positive, flags):
    a, b = feats(5, 3), feats(5, 3, 0.5)
    loss, rows = ops.info_nce_pair(a, b, tau=0.5, positive=positive, return_rows=True)
    (name, c), = lib.exports()
    assert name == "rlap_infonce_pair"
    assert (c["n"], c["F"], c["tau"], c["flags"]) == (5, 3, 0.5, flags)
    assert c["a"] == a.reshape(-1).tolist() and c["b"] == b.reshape(-1).tolist()
    assert loss.dim() == 0 and loss.dtype == torch.float64 and float(loss) == 1.5
    assert rows.shape == (2, 5) and rows.dtype == torch.float64 and bool((rows[0] == -1).all()) and bool((rows[1] == -3).all())
    assert ops.last_stats == {"rows": 5, "features": 3, "arena_bytes": ARENA, "parts": 7, "groups": 3, "host_syncs": 0}
    assert not loss.requires_grad


def test_defaults(lib):
    out = ops.info_nce_pair(feats(2, 2), feats(2, 2))
    (_, c), = lib.exports()
    assert (c["tau"], c["flags"]) == (0.4, 0) and isinstance(out, torch.Tensor) and out.dim() == 0


def test_non_contiguous_inputs_are_packed(lib):
    a = feats(3, 5).t()          # (5, 3), strided
    ops.info_nce_pair(a, a, tau=1.0)
    (_, c), = lib.exports()
    assert c["a"] == a.contiguous().reshape(-1).tolist() and (c["n"], c["F"]) == (5, 3)


BAD = [
    (torch.zeros(5), torch.zeros(5), 0.4, "scaled"),                                   # not 2-D
    (torch.zeros(1, 5, 3), torch.zeros(1, 5, 3), 0.4, "scaled"),
    (torch.zeros(5, 3), torch.zeros(5, 4), 0.4, "scaled"),                             # shapes differ
    (torch.zeros(5, 3), torch.zeros(4, 3), 0.4, "scaled"),
    (torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.float64), 0.4, "scaled"),   # not float32
    (torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.float16), 0.4, "scaled"),
    ([[1.0, 2.0]], torch.zeros(1, 2), 0.4, "scaled"),                                  # not a tensor
    (torch.zeros(0, 3), torch.zeros(0, 3), 0.4, "scaled"),                             # no row
    (torch.zeros(5, 0), torch.zeros(5, 0), 0.4, "scaled"),                             # no column
    (torch.zeros(2, 513), torch.zeros(2, 513), 0.4, "scaled"),                         # F > 512
    (torch.zeros(5, 3), torch.zeros(5, 3), 0.0, "scaled"),                             # tau outside [1/32, 1024]
    (torch.zeros(5, 3), torch.zeros(5, 3), 1025.0, "scaled"),
    (torch.zeros(5, 3), torch.zeros(5, 3), float("nan"), "scaled"),
    (torch.zeros(5, 3), torch.zeros(5, 3), "0.4", "scaled"),
    (torch.zeros(5, 3), torch.zeros(5, 3), True, "scaled"),
    (torch.zeros(5, 3), torch.zeros(5, 3), 0.4, "both"),                               # positive
    (torch.zeros(5, 3), torch.zeros(5, 3), 0.4, None),
]


@pytest.mark.parametrize("a,b,tau,positive", BAD)
def test_bad_arguments_raise_value_error_before_any_call(lib, monkeypatch, a, b, tau, positive):
    def reached(*args, **kw):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    with pytest.raises(ValueError):
        ops.info_nce_pair(a, b, tau=tau, positive=positive)
    if isinstance(a, torch.Tensor) and a.dim() == 2:
        with pytest.raises(ValueError):
            adapters.NodeContrast(tau=tau, positive=positive, pair=True)(a, b)
    assert lib.exports() == []


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (7, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    before = ops.last_stats
    with pytest.raises(exc, match=f"status {status}"):
        ops.info_nce_pair(feats(4, 2), feats(4, 2))
    assert ops.last_stats is before


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.info_nce_pair(feats(4, 2), feats(4, 2))
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_infonce_pair")
    assert names[i:i + 4] == ["rlap_infonce_pair", "rlap_workspace_needed", "rlap_set_workspace", "rlap_infonce_pair"]
    assert lib.calls[i + 2][1]["ws_bytes"] >= 1 << 20


@pytest.mark.parametrize("which", ["both", "anchor", "sample"])
def test_autograd_calls_the_backward_export_once_with_the_saved_z(lib, which):
    a = feats(4, 3).requires_grad_(which in ("both", "anchor"))
    b = feats(4, 3, 0.25).requires_grad_(which in ("both", "sample"))
    loss = ops.info_nce_pair(a, b, tau=0.5, positive="raw")
    assert loss.requires_grad
    (2.5 * loss).backward()
    (fname, f), (bname, c) = lib.exports()
    assert (fname, bname) == ("rlap_infonce_pair", "rlap_infonce_pair_backward")
    assert (c["n"], c["F"], c["tau"], c["flags"]) == (4, 3, 0.5, 1) == (f["n"], f["F"], f["tau"], f["flags"])
    assert c["a"] == a.detach().reshape(-1).tolist() and c["b"] == b.detach().reshape(-1).tolist()
    assert c["z"] == [2.0] * 4 + [5.0] * 4 and c["g"] == [2.5]      # Z then Zc as the forward left them; the upstream gradient
    if a.requires_grad:
        assert a.grad.shape == a.shape and a.grad.dtype == torch.float32 and bool((a.grad == 3).all())
    else:
        assert a.grad is None
    if b.requires_grad:
        assert bool((b.grad == 4).all())
    else:
        assert b.grad is None
    assert ops.last_stats["rows"] == 4 and ops.last_stats["host_syncs"] == 0


def test_rows_are_not_differentiable_and_no_graph_without_requires_grad(lib):
    a = feats(4, 3).requires_grad_(True)
    loss, rows = ops.info_nce_pair(a, feats(4, 3), return_rows=True)
    assert loss.requires_grad and not rows.requires_grad
    assert not ops.info_nce_pair(feats(4, 3), feats(4, 3)).requires_grad
    with torch.no_grad():
        assert not ops.info_nce_pair(a, a).requires_grad
    assert [c[0] for c in lib.exports()] == ["rlap_infonce_pair"] * 3


def test_pair_info_layout(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_infonce_pair_info", "InfoncePairInfo")
    assert [f for f, _ in _lib.InfoncePairInfo._fields_] == ["rows", "features", "arena_bytes", "parts", "groups", "host_syncs", "pad"]
    assert [f for f, _ in _lib.InfonceInfo._fields_] == ["rows", "features", "parts", "arena_bytes", "host_syncs", "pad"]   # left alone


def test_exports_are_declared():
    assert {"rlap_infonce_pair", "rlap_infonce_pair_backward"} <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "int rlap_infonce_pair(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags" in hdr
    assert "int rlap_infonce_pair_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags" in hdr
    lib = _lib.load()
    assert lib.rlap_infonce_pair.argtypes[-1]._type_ is _lib.InfoncePairInfo
    assert lib.rlap_infonce_pair_backward.argtypes[-1]._type_ is _lib.InfoncePairInfo


# ------------------------------------------------------------------------------------------------ the adapter
def test_node_contrast_pair_makes_one_call_of_each_export(lib):
    h1, h2 = feats(4, 3).requires_grad_(True), feats(4, 3, 0.5).requires_grad_(True)
    loss = adapters.NodeContrast(tau=0.5, pair=True)(h1, h2)
    assert float(loss.detach()) == 1.5 and loss.dtype == torch.float64
    (name, x), = lib.exports()
    assert name == "rlap_infonce_pair" and x["flags"] == 1 and x["tau"] == 0.5                  # "raw" by default
    assert x["a"] == h1.detach().reshape(-1).tolist() and x["b"] == h2.detach().reshape(-1).tolist()
    loss.backward()
    assert [c[0] for c in lib.exports()] == ["rlap_infonce_pair", "rlap_infonce_pair_backward"]
    assert lib.exports()[1][1]["g"] == [1.0]
    assert bool((h1.grad == 3).all()) and bool((h2.grad == 4).all())


def test_node_contrast_default_still_makes_two_calls_of_each(lib):
    h1, h2 = feats(4, 3).requires_grad_(True), feats(4, 3, 0.5).requires_grad_(True)
    contrast = adapters.NodeContrast(tau=0.5)
    assert contrast.pair is False
    contrast(h1, h2).backward()
    assert sorted(c[0] for c in lib.exports()) == ["rlap_infonce"] * 2 + ["rlap_infonce_backward"] * 2


def test_node_contrast_pair_takes_the_views_of_a_layer(lib):
    h = torch.stack([feats(4, 3), feats(4, 3, 0.5), feats(4, 3, 9.0)])
    adapters.NodeContrast(tau=0.4, positive="scaled", pair=True)(h)
    (name, x), = lib.exports()
    assert name == "rlap_infonce_pair" and x["a"] == h[0].reshape(-1).tolist() and x["b"] == h[1].reshape(-1).tolist() and x["flags"] == 0
    for bad in (feats(4, 3), h[:1]):
        with pytest.raises(ValueError):
            adapters.NodeContrast(pair=True)(bad)
