"""The fused Barlow Twins loss (ops.barlow_twins_loss, rlap_bt_loss / rlap_bt_loss_backward) without a GPU:

  * the rule -- the host mirror (tests/csrc/bt_mirror.cc, every value from rlap_amd/csrc/rlap_bt.h, contraction off) against a
    float64 torch restatement of the published bt_loss and its autograd, for lambd in {0, None = 1 / F, 1}, eps in {0, 1e-15, 1e-3}
    and both settings of `standardize`; the order's invariances; the exact properties; the special cases;
  * the index arithmetic of the header in a stand-alone program under -fsanitize=address,undefined, exhaustively for N <= 300;
  * the Python -> C mapping of both exports on a stub library, the layout of rlap_bt_info, adapters.BarlowTwinsContrast.

The bounds of the first group are four times the largest differences measured with these inputs (DESIGN 4.27 has the figures): the
rule's error is that of float32 standardised values and of float32 chains, a property of the formats and not of the seed.  Measured
here, over all 108 cases: loss and `on` 1.31e-7 relative (N = 33, F = 3, standardize=False; 1.19e-7 at (2, 1) standardised), `off`
2.05e-7 relative (N = 33, F = 3), gradients 1.92e-6 of the largest entry (N = 129, F = 512, lambd = 1, eps = 1e-3, where the
off-diagonal term, which passes through the float32 cross matrix and a float32 chain of length 512, carries the gradient).  Every
term is checked on its own.  At (N, F) = (2, 1) the standardised values are +-1/sqrt(2) whatever h is, so c = +-1/2 and every
gradient is zero up to eps: there the gradients are bounded relative to g * 2 |1 - c| / (N sd), the size of the terms that cancel
in dh (measured 3.13e-8 of it), and `off`, a sum over no entry, is exactly 0 on both sides.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import bt_mirror as bm
import cca_mirror as cm
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, f64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_BOUND = 4 * 1.32e-7     # relative to the loss (a sum of squares: nothing cancels)
ON_BOUND = 4 * 1.32e-7       # |on - reference|, relative to on
OFF_BOUND = 4 * 2.06e-7      # |off - reference|, relative to off
GRAD_BOUND = 4 * 1.92e-6     # relative to the largest gradient entry (or to the cancelling terms at N = 2)
G_UP = 0.75


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return bm.build(tmp_path_factory.mktemp("bt"))


# ------------------------------------------------------------------------------------------------ the rule
SHAPES = [(2, 1), (33, 3), (65, 33), (300, 100), (129, 512), (2708, 64)]
GPU_SHAPES = [(2, 1), (3, 2), (31, 31), (32, 32), (33, 3), (64, 64), (65, 65), (65, 100), (255, 128), (257, 129), (300, 256), (257, 300),
              (300, 512), (300, 1), (2708, 33)]   # tests/test_gpu_bt.py's, with its seeds


def reference(n, f, seed, cache={}):
    """The float64 cross-correlation of a shape's inputs, computed once."""
    key = (n, f, seed)
    if key not in cache:
        a, b = bm.views(n, f, seed)
        cache[key] = bm.restatement(a, b)[3]
    return cache[key]


SEEDED = [(n, f, 1000 + n) for n, f in SHAPES] + [(n, f, 4000 + 7 * n + f) for n, f in GPU_SHAPES]


@pytest.mark.parametrize("n,f,seed", [s for s in SEEDED if s[0] >= 31 and s[1] >= 3])
def test_the_inputs_are_far_from_symmetric(n, f, seed):
    """A kernel that computes the transpose, or the upper triangle mirrored, must not pass: the float64 cross-correlation of
    every input with N >= 31 and F >= 3 differs from its transpose by at least 0.5 somewhere."""
    c = reference(n, f, seed)
    gap = np.abs(c - c.T).max()
    print(f"n={n} F={f}: max |c_kl - c_lk| = {gap:.3f}")
    assert gap >= 0.5


@pytest.mark.parametrize("standardize", [True, False])
@pytest.mark.parametrize("eps", [0.0, 1e-15, 1e-3])
@pytest.mark.parametrize("lambd", [0.0, None, 1.0])
@pytest.mark.parametrize("n,f", SHAPES)
def test_mirror_against_the_float64_restatement(mirror, n, f, lambd, eps, standardize):
    a, b = bm.views(n, f, 1000 + n)
    m = bm.run(mirror, a, b, lambd, eps, standardize, g=G_UP)
    terms, ga, gb, c = bm.restatement(a, b, lambd, eps, standardize, g=G_UP)
    loss, on, off = terms
    rel = abs(m["loss"] - loss) / abs(loss)
    onrel = abs(m["on"] - on) / on
    gmax = max(np.abs(ga).max(), np.abs(gb).max())
    if n == 2 and standardize:                                 # every gradient cancels, see the top
        sd_min = min(m["colstat"][f:2 * f].min(), m["colstat"][3 * f:].min())
        gscale = G_UP * 2 * abs(1 - c[0, 0]) / (n * sd_min)
    else:
        gscale = gmax
    grel = max(np.abs(m["ga"] - ga).max(), np.abs(m["gb"] - gb).max()) / gscale
    print(f"n={n} F={f} lambd={lambd} eps={eps} standardize={standardize}: loss {loss:.6g} rel {rel:.3g}, on rel {onrel:.3g}, "
          f"off {off:.6g} abs {abs(m['off'] - off):.3g}, gradients rel {grel:.3g}")
    assert rel <= LOSS_BOUND
    assert onrel <= ON_BOUND
    if f == 1:
        assert m["off"] == 0.0 and off == 0.0
    else:
        assert abs(m["off"] - off) <= OFF_BOUND * off
    assert grel <= GRAD_BOUND
    assert np.abs(m["cross"] - c).max() <= 2.0 ** -21 * max(1.0, np.abs(c).max())


# ------------------------------------------------------------------------------------------------ exact properties
def same(x, y):
    return np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


@pytest.mark.parametrize("n,f", [(33, 3), (65, 33), (300, 20)])
def test_with_eps_zero_the_standardisation_is_the_cca_mirrors(mirror, tmp_path_factory, n, f):
    """colstat against the CCA mirror's, bit for bit; z against cca::zval -- (float)(((double)h - mean) / sd), IEEE operations
    only, which numpy computes to the same bits from the CCA mirror's statistics (that mirror returns no z)."""
    cca = cm.build(tmp_path_factory.mktemp("cca"))
    a, b = bm.views(n, f, 21)
    m = bm.run(mirror, a, b, eps=0.0)
    want = cm.run(cca, a, b, 1e-3)
    assert same(m["colstat"], want["colstat"])
    for v, x in enumerate((a, b)):
        mean, sd = want["colstat"][2 * f * v:2 * f * v + f], want["colstat"][2 * f * v + f:2 * f * v + 2 * f]
        assert same(m["z"][v], ((x.astype(np.float64) - mean) / sd).astype(np.float32))
    assert same(bm.run(mirror, a, b, eps=1e-15)["colstat"], m["colstat"])       # eps enters z alone
    assert not same(bm.run(mirror, a, b, eps=1e-3)["z"], m["z"])


@pytest.mark.parametrize("n,f", [(65, 33), (300, 20)])
def test_threads_and_tiling_change_no_bit(mirror, n, f):
    """The mirror computes every cross entry and every row of P on its own, so `block` and `threads` only change how they are
    grouped and dealt out: this pins the mirror, not the kernels.  The guard against an order that depends on the grid is the
    bit-for-bit comparison on the device (tests/test_gpu_bt.py: several parts, several workgroups per part)."""
    a, b = bm.views(n, f, 7)
    base = bm.run(mirror, a, b, g=1.0, block=32, threads=8)
    for block, threads in ((1, 8), (7, 3), (128, 1), (1000, 8)):
        other = bm.run(mirror, a, b, g=1.0, block=block, threads=threads)
        for key in ("terms", "colstat", "cross", "z", "ga", "gb"):
            assert same(base[key], other[key]), (block, threads, key)


@pytest.mark.parametrize("f", [3, 32, 33])
def test_zero_columns_behind_the_padded_image_change_no_bit(mirror, f):
    a, b = bm.views(65, f, 11)
    m = bm.run(mirror, a, b, g=1.0)
    for pad in (1, 3):
        w = bm.run(mirror, a, b, g=1.0, pad_tiles=pad)
        for key in ("terms", "colstat", "cross", "ga", "gb"):
            assert same(m[key], w[key]), (pad, key)


def test_parts_depend_on_n_and_f_alone(mirror):
    for n in (2, 32, 33, 300, 2708, 34493, 169343):
        for f in (1, 64, 100, 512):
            p = mirror.bt_parts(n, f)
            tiles = (n + 31) // 32
            assert 1 <= p <= min(tiles, 64) and mirror.bt_part_begin(n, f, 0) == 0 and mirror.bt_part_begin(n, f, p) == 32 * tiles
            assert all(mirror.bt_part_begin(n, f, q) % 32 == 0 for q in range(p + 1))
    assert mirror.bt_parts(2708, 64) == 64 and mirror.bt_parts(300, 512) == 10 and mirror.bt_parts(169343, 512) == 16
    assert mirror.bt_parts(169343, 256) == 64 and mirror.bt_parts(169343, 300) == 26
    assert [mirror.bt_pair_groups(f) for f in (1, 64, 65, 128, 256, 300, 512)] == [1, 1, 2, 2, 4, 10, 16]
    assert [mirror.bt_row_groups(f) for f in (1, 128, 256, 257, 512)] == [1, 1, 1, 2, 2]
    assert [mirror.bt_cross_instance(t) for t in range(0, 18)] == [0, 1, 1, 2, 2] + [4] * 12 + [0]


def test_lambd_zero_is_the_diagonal_term_alone(mirror):
    a, b = bm.views(65, 33, 17)
    m = bm.run(mirror, a, b, lambd=0.0, g=G_UP)
    assert same(m["terms"][0], m["terms"][1]) and m["off"] > 0                  # loss == on
    big = bm.run(mirror, a, b, lambd=1.0, g=G_UP)
    assert same(big["terms"][1:], m["terms"][1:]) and not same(big["ga"], m["ga"]) and big["loss"] > m["loss"]


@pytest.mark.parametrize("n,f", [(33, 3), (65, 33), (300, 100)])
def test_the_swapped_call_is_the_transpose(mirror, n, f):
    """c(h2, h1) = c(h1, h2)^T bit for bit (the product of two floats commutes, the chains run over the same rows), `on` reads the
    same diagonal in the same order, `off` adds the same non-negative terms in another order: at most F^2 roundings of 2^-53 each
    on either side."""
    a, b = bm.views(n, f, 23)
    m, s = bm.run(mirror, a, b, g=G_UP), bm.run(mirror, b, a, g=G_UP)
    assert same(s["cross"], m["cross"].T) and not same(m["cross"], m["cross"].T)
    assert same(s["on"], m["on"])
    assert abs(s["off"] - m["off"]) <= 2 * f * f * 2.0 ** -53 * m["off"]
    assert same(s["colstat"][:2 * f], m["colstat"][2 * f:]) and same(s["colstat"][2 * f:], m["colstat"][:2 * f])


def test_a_constant_column_is_finite_forward_and_nan_in_its_own_gradient(mirror):
    """A column that is constant with an exactly representable mean has sd = 0 exactly: with eps > 0 its z is +0, the loss is
    finite, and dh is NaN in that column alone (0 * 0 * inf); with eps = 0 its z is NaN (0 / 0, as in cca_loss): the terms, that
    column of dh1 and all of dh2, which sums over it, are NaN.  What torch gives is not asserted."""
    a, b = bm.views(40, 5, 19)
    a[:, 2] = 1.5
    m = bm.run(mirror, a, b, g=1.0)
    assert m["colstat"][2] == 1.5 and m["colstat"][5 + 2] == 0.0
    assert same(m["z"][0][:, 2], np.zeros(40, dtype=np.float32))                # +0, not -0
    assert np.isfinite(m["terms"]).all() and np.isfinite(m["cross"]).all() and same(m["cross"][2], np.zeros(5, dtype=np.float32))
    assert np.isnan(m["ga"][:, 2]).all() and np.isfinite(np.delete(m["ga"], 2, axis=1)).all() and np.isfinite(m["gb"]).all()
    z = bm.run(mirror, a, b, eps=0.0, g=1.0)
    assert np.isnan(z["terms"]).all() and np.isnan(z["ga"][:, 2]).all() and np.isnan(z["gb"]).all()
    assert np.isfinite(np.delete(z["ga"], 2, axis=1)).all()
    plain = bm.run(mirror, a, b, standardize=False, g=1.0)                      # nothing divides
    assert np.isfinite(plain["terms"]).all() and np.isfinite(plain["ga"]).all() and np.isnan(plain["colstat"]).all()


def test_without_the_standardisation_z_is_h(mirror):
    a, b = bm.views(65, 33, 29)
    m = bm.run(mirror, a, b, standardize=False, g=G_UP)
    assert same(m["z"][0], a) and same(m["z"][1], b) and np.isnan(m["colstat"]).all()       # colstat is left as it was
    for eps in (0.0, 1e-3):
        other = bm.run(mirror, a, b, eps=eps, standardize=False, g=G_UP)
        for key in ("terms", "cross", "ga", "gb"):
            assert same(m[key], other[key]), (eps, key)


def test_ranges(mirror):
    assert all(mirror.bt_lambd_ok(x) and mirror.bt_eps_ok(x) for x in (0.0, 1e-15, 1e-3, 1.0, 1e300))
    assert not any(mirror.bt_lambd_ok(x) or mirror.bt_eps_ok(x) for x in (-1e-9, -1.0, float("nan"), float("inf")))
    assert mirror.bt_flags_ok(0) and mirror.bt_flags_ok(1) and not mirror.bt_flags_ok(2) and not mirror.bt_flags_ok(3)


# ------------------------------------------------------------------------------------------------ the index arithmetic, under the sanitizers
def test_the_index_arithmetic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "bt_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "bt_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "300 sizes, 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_bt_loss": "h a b n F lambd eps flags terms colstat cross info",
    "rlap_bt_loss_backward": "h a b n F lambd eps flags colstat cross g ga gb info",
}
ARENA = 9876
TERMS = [1.5, 2.0, 3.0]


def f32_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


class BtStub(StubLib):
    """Records both exports; the forward writes terms = 1.5, 2, 3, colstat = 0.5 and cross = 0.25; the backward ga = 3, gb = 4."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        status = self.statuses.pop(0) if self.statuses else self.status
        n, F = a["n"], a["F"]
        rec = {k: a[k] for k in ("n", "F", "lambd", "eps", "flags")}
        rec["a"], rec["b"] = f32_at(a["a"], n * F), f32_at(a["b"], n * F)
        back = name.endswith("backward")
        if back:
            rec["colstat"], rec["cross"], rec["g"] = f64_at(a["colstat"], 4 * F), f32_at(a["cross"], F * F), f64_at(a["g"], 1)
        self.calls.append((name, rec))
        if status:
            return status
        if back:
            for key, v in (("ga", 3.0), ("gb", 4.0)):
                out = ctypes.cast(a[key], ctypes.POINTER(ctypes.c_float))
                for i in range(n * F):
                    out[i] = v
        else:
            assert a["colstat"] == a["terms"] + 32                        # one buffer: terms (and a spare slot) | colstat
            out = ctypes.cast(a["terms"], ctypes.POINTER(ctypes.c_double))
            for i, v in enumerate(TERMS + [-1.0] + [0.5] * (4 * F)):
                out[i] = v
            out = ctypes.cast(a["cross"], ctypes.POINTER(ctypes.c_float))
            for i in range(F * F):
                out[i] = 0.25
        info = a["info"]._obj
        info.rows, info.features, info.parts, info.arena_bytes, info.host_syncs = n, F, 7, ARENA, 0
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, BtStub())


def feats(n, f, shift=0.0):
    return (torch.arange(n * f, dtype=torch.float32).reshape(n, f) / 4.0 - 1.0 + shift)


def test_arguments_of_the_forward_export(lib):
    a, b = feats(5, 3), feats(5, 3, 0.5)
    out = ops.barlow_twins_loss(a, b, lambd=0.5, eps=1e-3, return_terms=True)
    (name, c), = lib.exports()
    assert name == "rlap_bt_loss"
    assert (c["n"], c["F"], c["lambd"], c["eps"], c["flags"]) == (5, 3, 0.5, 1e-3, 0)
    assert c["a"] == a.reshape(-1).tolist() and c["b"] == b.reshape(-1).tolist()
    assert len(out) == 3 and all(t.dim() == 0 and t.dtype == torch.float64 for t in out) and [float(t) for t in out] == TERMS
    assert ops.last_stats == {"rows": 5, "features": 3, "parts": 7, "arena_bytes": ARENA, "host_syncs": 0}
    assert not out[0].requires_grad


def test_defaults(lib):
    out = ops.barlow_twins_loss(feats(2, 4), feats(2, 4))
    (_, c), = lib.exports()
    assert (c["lambd"], c["eps"], c["flags"]) == (0.25, 1e-15, 0) and isinstance(out, torch.Tensor) and out.dim() == 0 and float(out) == 1.5


def test_standardize_false_is_flag_bit_zero(lib):
    a = feats(4, 3).requires_grad_(True)
    ops.barlow_twins_loss(a, feats(4, 3), standardize=False).backward()
    (_, f), (_, c) = lib.exports()
    assert f["flags"] == 1 == c["flags"] == _lib_flag()


def _lib_flag():
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "enum { RLAP_BT_NO_STANDARDIZE = 1 };" in hdr
    return ops.BT_NO_STANDARDIZE


def test_non_contiguous_inputs_are_packed(lib):
    a = feats(3, 5).t()          # (5, 3), strided
    ops.barlow_twins_loss(a, a, lambd=1.0)
    (_, c), = lib.exports()
    assert c["a"] == a.contiguous().reshape(-1).tolist() and (c["n"], c["F"]) == (5, 3)


GOOD = {"lambd": None, "eps": 1e-15, "standardize": True}
BAD = [
    (torch.zeros(5), torch.zeros(5), {}),                                      # not 2-D
    (torch.zeros(1, 5, 3), torch.zeros(1, 5, 3), {}),
    (torch.zeros(5, 3), torch.zeros(5, 4), {}),                                # shapes differ
    (torch.zeros(5, 3), torch.zeros(4, 3), {}),
    (torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.float64), {}),   # not float32
    (torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.float16), {}),
    (torch.zeros(5, 3, dtype=torch.bfloat16), torch.zeros(5, 3, dtype=torch.bfloat16), {}),
    (torch.zeros(5, 3, dtype=torch.int64), torch.zeros(5, 3, dtype=torch.int64), {}),
    ([[1.0, 2.0], [3.0, 4.0]], torch.zeros(2, 2), {}),                         # not a tensor
    (torch.zeros(5, 3), torch.zeros(5, 3, device="meta"), {}),                 # two devices
    (torch.zeros(0, 3), torch.zeros(0, 3), {}),                                # N < 2
    (torch.zeros(1, 3), torch.zeros(1, 3), {}),
    (torch.zeros(5, 0), torch.zeros(5, 0), {}),                                # no column
    (torch.zeros(2, 513), torch.zeros(2, 513), {}),                            # F > 512
    (torch.zeros(5, 3), torch.zeros(5, 3), {"lambd": -1e-3}),                  # lambd negative, not finite, not a number
    (torch.zeros(5, 3), torch.zeros(5, 3), {"lambd": float("nan")}),
    (torch.zeros(5, 3), torch.zeros(5, 3), {"lambd": float("inf")}),
    (torch.zeros(5, 3), torch.zeros(5, 3), {"lambd": "1e-3"}),
    (torch.zeros(5, 3), torch.zeros(5, 3), {"lambd": True}),
    (torch.zeros(5, 3), torch.zeros(5, 3), {"eps": -1e-15}),                   # eps likewise
    (torch.zeros(5, 3), torch.zeros(5, 3), {"eps": float("nan")}),
    (torch.zeros(5, 3), torch.zeros(5, 3), {"eps": float("inf")}),
    (torch.zeros(5, 3), torch.zeros(5, 3), {"eps": None}),
    (torch.zeros(5, 3), torch.zeros(5, 3), {"eps": False}),
    (torch.zeros(5, 3), torch.zeros(5, 3), {"standardize": 1}),                # standardize not a bool
    (torch.zeros(5, 3), torch.zeros(5, 3), {"standardize": None}),
]


@pytest.mark.parametrize("a,b,kw", BAD)
def test_bad_arguments_raise_value_error_before_any_call(lib, monkeypatch, a, b, kw):
    def reached(*args, **kwargs):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    with pytest.raises(ValueError):
        ops.barlow_twins_loss(a, b, **dict(GOOD, **kw))
    assert lib.exports() == []


def test_the_ends_of_the_ranges_are_inside(lib):
    ops.barlow_twins_loss(feats(2, 512), feats(2, 512), lambd=0, eps=0)
    (_, c), = lib.exports()
    assert (c["n"], c["F"], c["lambd"], c["eps"]) == (2, 512, 0.0, 0.0)


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (7, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    before = ops.last_stats
    with pytest.raises(exc, match=f"status {status}"):
        ops.barlow_twins_loss(feats(4, 2), feats(4, 2))
    assert ops.last_stats is before


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.barlow_twins_loss(feats(4, 2), feats(4, 2))
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_bt_loss")
    assert names[i:i + 4] == ["rlap_bt_loss", "rlap_workspace_needed", "rlap_set_workspace", "rlap_bt_loss"]
    assert lib.calls[i + 2][1]["ws_bytes"] >= 1 << 20


@pytest.mark.parametrize("which", ["both", "first", "second"])
def test_autograd_calls_the_backward_export_once(lib, which):
    a = feats(4, 3).requires_grad_(which in ("both", "first"))
    b = feats(4, 3, 0.25).requires_grad_(which in ("both", "second"))
    loss = ops.barlow_twins_loss(a, b, lambd=0.5, eps=1e-3)
    assert loss.requires_grad
    (2.5 * loss).backward()
    (fname, f), (bname, c) = lib.exports()
    assert (fname, bname) == ("rlap_bt_loss", "rlap_bt_loss_backward")
    assert (c["n"], c["F"], c["lambd"], c["eps"], c["flags"]) == (4, 3, 0.5, 1e-3, 0) == (f["n"], f["F"], f["lambd"], f["eps"], f["flags"])
    assert c["a"] == a.detach().reshape(-1).tolist() and c["b"] == b.detach().reshape(-1).tolist()
    assert c["colstat"] == [0.5] * 12 and c["cross"] == [0.25] * 9 and c["g"] == [2.5]   # the forward's; the upstream gradient, on the device
    if a.requires_grad:
        assert a.grad.shape == a.shape and a.grad.dtype == torch.float32 and bool((a.grad == 3).all())
    else:
        assert a.grad is None
    if b.requires_grad:
        assert bool((b.grad == 4).all())
    else:
        assert b.grad is None
    assert ops.last_stats["rows"] == 4 and ops.last_stats["host_syncs"] == 0


def test_the_terms_are_not_differentiable(lib):
    a = feats(4, 3).requires_grad_(True)
    loss, on, off = ops.barlow_twins_loss(a, feats(4, 3), return_terms=True)
    assert loss.requires_grad and not (on.requires_grad or off.requires_grad)
    assert [float(t.detach()) for t in (loss, on, off)] == TERMS


def test_no_graph_is_recorded_without_requires_grad(lib):
    assert not ops.barlow_twins_loss(feats(4, 3), feats(4, 3)).requires_grad
    a = feats(4, 3).requires_grad_(True)
    with torch.no_grad():
        assert not ops.barlow_twins_loss(a, a).requires_grad
    assert [c[0] for c in lib.exports()] == ["rlap_bt_loss"] * 2


def test_bt_info_layout(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_bt_info", "BtInfo")
    assert [f for f, _ in _lib.BtInfo._fields_] == ["rows", "features", "parts", "arena_bytes", "host_syncs", "pad"]


def test_exports_are_declared():
    assert {"rlap_bt_loss", "rlap_bt_loss_backward"} <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    doc = hdr[hdr.index("The fused Barlow Twins loss"):hdr.index("} rlap_bt_info;")]
    assert "RLAP_BT_NO_STANDARDIZE" in doc and "zero variance" in doc
    api = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_api.hip")).read()
    assert "bt::flags_ok(flags)" in api[api.index("int bt_check("):api.index("int rlap_bt_loss(")]


# ------------------------------------------------------------------------------------------------ the adapter
def test_barlow_twins_contrast_takes_two_embeddings(lib):
    h1, h2 = feats(4, 3).requires_grad_(True), feats(4, 3, 0.5).requires_grad_(True)
    loss = adapters.BarlowTwinsContrast(lambd=0.5, eps=1e-3)(h1, h2)
    assert float(loss.detach()) == 1.5 and loss.dtype == torch.float64 and loss.dim() == 0
    (_, c), = lib.exports()                                               # ONE call, not loss(h1, h2) and loss(h2, h1)
    assert (c["lambd"], c["eps"]) == (0.5, 1e-3) and c["a"] == h1.detach().reshape(-1).tolist() and c["b"] == h2.detach().reshape(-1).tolist()
    loss.backward()
    assert bool((h1.grad == 3).all()) and bool((h2.grad == 4).all())
    m = adapters.BarlowTwinsContrast()
    assert m.lambd is None and m.eps == 1e-15 and "ONE call" in adapters.BarlowTwinsContrast.__doc__


def test_barlow_twins_contrast_takes_the_views_of_a_layer(lib):
    h = torch.stack([feats(4, 3), feats(4, 3, 0.5), feats(4, 3, 9.0)])
    adapters.BarlowTwinsContrast()(h)
    (_, c), = lib.exports()
    assert c["a"] == h[0].reshape(-1).tolist() and c["b"] == h[1].reshape(-1).tolist() and c["lambd"] == 1.0 / 3 and c["eps"] == 1e-15
    for bad in (feats(4, 3), h[:1]):
        with pytest.raises(ValueError):
            adapters.BarlowTwinsContrast()(bad)
