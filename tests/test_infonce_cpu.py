"""The fused InfoNCE loss (ops.info_nce, rlap_infonce / rlap_infonce_backward) without a GPU:

  * the rule -- the host mirror (tests/csrc/infonce_mirror.cc, every value from rlap_amd/csrc/rlap_infonce.h, contraction off) against
    a float64 torch restatement of the reference's two losses and their autograd, for both `positive` settings and tau in
    {1/32, 0.4, 2}; expw against float64 exp on a dense grid over [-64, 0]; the order's invariances;
  * the index arithmetic of the header in a stand-alone program under -fsanitize=address,undefined, exhaustively for N <= 300;
  * the Python -> C mapping of both exports on a stub library, the layout of rlap_infonce_info, adapters.NodeContrast.

The bounds of the first group are four times the largest differences measured with these inputs (DESIGN 4.15 has the figures): the
rule's error is that of float32 chains of length F and of a float32 exponential, a property of the formats and not of the seed.
Measured here: loss 2.19e-7 relative (tau = 1/32, F = 512, where a rounding of s is multiplied by 32 before the exponential),
gradients 1.76e-6 of the largest entry; expw 7.63e-8 relative (1.28 units of 2^-24).  The inputs are two views with cosine about 0.3
between positives, so that every loss is of order 0.1 to 30 and its relative error means something: a loss that cancels to 1e-7 keeps
an absolute error near 1e-9, which no relative bound describes.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import infonce_mirror as im
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, f64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_BOUND = 4 * 2.19e-7     # relative to the loss; never above 1e-5
GRAD_BOUND = 4 * 1.76e-6     # relative to the largest gradient entry
EXPW_BOUND = 4 * 7.63e-8     # relative
assert LOSS_BOUND <= 1e-5


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return im.build(tmp_path_factory.mktemp("infonce"))


def views(n, f, seed):
    """Two float32 views whose positives have cosine about 0.3."""
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((n, f)).astype(np.float32)
    b = (0.3 * a + rng.standard_normal((n, f))).astype(np.float32)
    return a, b


# ------------------------------------------------------------------------------------------------ the rule
SHAPES = [(33, 3), (65, 33), (300, 100), (129, 512)]


@pytest.mark.parametrize("tau", [1.0 / 32.0, 0.4, 2.0])
@pytest.mark.parametrize("positive", ["scaled", "raw"])
@pytest.mark.parametrize("n,f", SHAPES)
def test_mirror_against_the_float64_restatement(mirror, n, f, positive, tau):
    a, b = views(n, f, 1000 + n)
    g = 0.75
    m = im.run(mirror, a, b, tau, positive, g=g)
    loss, ga, gb = im.restatement(a, b, tau, positive, g=g)
    rel = abs(m["loss"] - loss) / abs(loss)
    gmax = max(np.abs(ga).max(), np.abs(gb).max())
    grel = max(np.abs(m["ga"] - ga).max(), np.abs(m["gb"] - gb).max()) / gmax
    print(f"n={n} F={f} {positive} tau={tau}: loss {loss:.6g} rel {rel:.3g}, gradients rel {grel:.3g}")
    assert 0.05 < abs(loss) < 50.0                                # the relative error is meaningful
    assert rel <= LOSS_BOUND
    assert grel <= GRAD_BOUND
    assert np.isfinite(m["rows"]).all() and abs(-m["rows"].mean() - loss) <= LOSS_BOUND * abs(loss)


def test_raw_and_scaled_differ_in_the_positive_term_alone(mirror):
    a, b = views(65, 33, 5)
    s = im.run(mirror, a, b, 0.4, "scaled")
    r = im.run(mirror, a, b, 0.4, "raw")
    assert s["z"].tobytes() == r["z"].tobytes() and s["sii"].tobytes() == r["sii"].tobytes()
    want = s["rows"] - (1.0 / 0.4 - 1.0) * s["sii"].astype(np.float64)
    assert np.abs(r["rows"] - want).max() < 1e-12


def test_expw_against_float64_exp(mirror):
    x = np.linspace(-64.0, 0.0, 2_000_001).astype(np.float32)
    y = im.expw(mirror, x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    rel = (np.abs(y - ref) / ref).max()
    print(f"expw: largest relative error {rel:.4g} over {x.size} points of [-64, 0]")
    assert rel <= EXPW_BOUND
    assert np.float32(mirror.infonce_expw(0.0)).tobytes() == np.float32(1.0).tobytes()
    assert (y > 2.0 ** -126).all() and (np.diff(y) >= 0).all()     # normal, and monotone on the grid


def test_tau_range(mirror):
    assert all(mirror.infonce_tau_ok(t) for t in (1.0 / 32.0, 0.4, 2.0, 1024.0))
    assert not any(mirror.infonce_tau_ok(t) for t in (0.0, 0.03, -0.4, 1024.5, float("nan"), float("inf")))


# ------------------------------------------------------------------------------------------------ order and invariance
@pytest.mark.parametrize("n,f", [(65, 33), (300, 20)])
def test_row_tiling_changes_no_bit(mirror, n, f):
    """The mirror computes every row on its own, so `block_rows` only changes how rows are grouped and dealt to threads: this pins
    the mirror, not the kernels.  The guard against an order that depends on the grid is the bit-for-bit comparison on the device
    (tests/test_gpu_infonce.py, N = 2708: twelve parts, hundreds of workgroups)."""
    a, b = views(n, f, 7)
    base = im.run(mirror, a, b, 0.4, "raw", g=1.0, block_rows=32)
    for block in (1, 7, 128, 1000):
        other = im.run(mirror, a, b, 0.4, "raw", g=1.0, block_rows=block)
        for key in ("loss", "z", "rows", "sii", "ga", "gb"):
            assert np.asarray(base[key]).tobytes() == np.asarray(other[key]).tobytes(), (block, key)


def test_parts_depend_on_n_alone(mirror):
    for n in (1, 32, 33, 300, 2708, 34493, 169343):
        p = mirror.infonce_parts(n)
        tiles = (n + 31) // 32
        assert 1 <= p <= tiles and mirror.infonce_part_begin(n, 0) == 0 and mirror.infonce_part_begin(n, p) == tiles
    assert mirror.infonce_parts(2708) > 1 and mirror.infonce_parts(169343) == 1
    assert [mirror.infonce_reg_row(r, 0) for r in range(16)] == [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19, 24, 25, 26, 27]
    assert [mirror.infonce_reg_row(r, 1) for r in range(16)] == [4, 5, 6, 7, 12, 13, 14, 15, 20, 21, 22, 23, 28, 29, 30, 31]


@pytest.mark.parametrize("f,pad", [(3, 1), (31, 1), (32, 32), (33, 31)])
def test_zero_feature_columns_change_no_bit(mirror, f, pad):
    a, b = views(65, f, 11)
    wide = lambda x: np.concatenate([x, np.zeros((x.shape[0], pad), dtype=np.float32)], axis=1)
    m = im.run(mirror, a, b, 0.4, "scaled", g=1.0)
    w = im.run(mirror, wide(a), wide(b), 0.4, "scaled", g=1.0)
    for key in ("loss", "z", "rows"):
        assert np.asarray(m[key]).tobytes() == np.asarray(w[key]).tobytes(), key
    for key in ("ga", "gb"):
        assert m[key].tobytes() == w[key][:, :f].tobytes() and not w[key][:, f:].any(), key


def test_a_zero_row_gives_finite_values(mirror):
    a, b = views(40, 5, 13)
    a[3] = 0.0
    b[17] = 0.0
    m = im.run(mirror, a, b, 0.4, "raw", g=1.0)
    for key in ("loss", "z", "rows", "ga", "gb"):
        assert np.isfinite(np.asarray(m[key])).all(), key
    assert m["sii"][3] == 0.0 and m["sii"][17] == 0.0
    loss, _, _ = im.restatement(a, b, 0.4, "raw")
    assert abs(m["loss"] - loss) <= LOSS_BOUND * abs(loss)


# ------------------------------------------------------------------------------------------------ the index arithmetic, under the sanitizers
def test_the_index_arithmetic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "infonce_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "infonce_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "300 sizes, 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_infonce": "h a b n F tau flags loss rows z info",
    "rlap_infonce_backward": "h a b n F tau flags z g ga gb info",
}
ARENA = 9876


def f32_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


class InfonceStub(StubLib):
    """Records both exports; the forward writes loss = 1.5, rows = -1, z = 2; the backward ga = 3, gb = 4."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        status = self.statuses.pop(0) if self.statuses else self.status
        n, F = a["n"], a["F"]
        rec = {k: a[k] for k in ("n", "F", "tau", "flags")}
        rec["a"], rec["b"] = f32_at(a["a"], n * F), f32_at(a["b"], n * F)
        back = name.endswith("backward")
        if back:
            rec["z"], rec["g"] = f64_at(a["z"], n), f64_at(a["g"], 1)
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
            assert a["rows"] == a["loss"] + 8 and a["z"] == a["loss"] + 8 * (1 + n)    # one buffer: loss | rows | z
            for key, v in (("rows", -1.0), ("z", 2.0)):
                out = ctypes.cast(a[key], ctypes.POINTER(ctypes.c_double))
                for i in range(n):
                    out[i] = v
        info = a["info"]._obj
        info.rows, info.features, info.parts, info.arena_bytes, info.host_syncs = n, F, 7, ARENA, 0
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, InfonceStub())


def feats(n, f, shift=0.0):
    return (torch.arange(n * f, dtype=torch.float32).reshape(n, f) / 4.0 - 1.0 + shift)


@pytest.mark.parametrize("positive,flags", [("scaled", 0), ("raw", 1)])
def test_arguments_of_the_forward_export(lib, positive, flags):
    a, b = feats(5, 3), feats(5, 3, 0.5)
    loss, rows = ops.info_nce(a, b, tau=0.5, positive=positive, return_rows=True)
    (name, c), = lib.exports()
    assert name == "rlap_infonce"
    assert (c["n"], c["F"], c["tau"], c["flags"]) == (5, 3, 0.5, flags)
    assert c["a"] == a.reshape(-1).tolist() and c["b"] == b.reshape(-1).tolist()
    assert loss.dim() == 0 and loss.dtype == torch.float64 and float(loss) == 1.5
    assert rows.shape == (5,) and rows.dtype == torch.float64 and bool((rows == -1).all())
    assert ops.last_stats == {"rows": 5, "features": 3, "parts": 7, "arena_bytes": ARENA, "host_syncs": 0}
    assert not loss.requires_grad


def test_defaults(lib):
    out = ops.info_nce(feats(2, 2), feats(2, 2))
    (_, c), = lib.exports()
    assert (c["tau"], c["flags"]) == (0.4, 0) and isinstance(out, torch.Tensor) and out.dim() == 0
    assert _lib.INFONCE_POSITIVE_RAW == 1


def test_non_contiguous_inputs_are_packed(lib):
    a = feats(3, 5).t()          # (5, 3), strided
    ops.info_nce(a, a, tau=1.0)
    (_, c), = lib.exports()
    assert c["a"] == a.contiguous().reshape(-1).tolist() and (c["n"], c["F"]) == (5, 3)


BAD = [
    (torch.zeros(5), torch.zeros(5), 0.4, "scaled"),                                   # not 2-D
    (torch.zeros(1, 5, 3), torch.zeros(1, 5, 3), 0.4, "scaled"),
    (torch.zeros(5, 3), torch.zeros(5, 4), 0.4, "scaled"),                             # shapes differ
    (torch.zeros(5, 3), torch.zeros(4, 3), 0.4, "scaled"),
    (torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.float64), 0.4, "scaled"),   # not float32
    (torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.float16), 0.4, "scaled"),
    (torch.zeros(5, 3, dtype=torch.int64), torch.zeros(5, 3, dtype=torch.int64), 0.4, "scaled"),
    ([[1.0, 2.0]], torch.zeros(1, 2), 0.4, "scaled"),                                  # not a tensor
    (torch.zeros(0, 3), torch.zeros(0, 3), 0.4, "scaled"),                             # no row
    (torch.zeros(5, 0), torch.zeros(5, 0), 0.4, "scaled"),                             # no column
    (torch.zeros(2, 513), torch.zeros(2, 513), 0.4, "scaled"),                         # F > 512
    (torch.zeros(5, 3), torch.zeros(5, 3), 0.0, "scaled"),                             # tau outside [1/32, 1024]
    (torch.zeros(5, 3), torch.zeros(5, 3), 0.03, "scaled"),
    (torch.zeros(5, 3), torch.zeros(5, 3), 1025.0, "scaled"),
    (torch.zeros(5, 3), torch.zeros(5, 3), -0.4, "scaled"),
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
        ops.info_nce(a, b, tau=tau, positive=positive)
    assert lib.exports() == []


def test_the_ends_of_tau_are_inside(lib):
    ops.info_nce(feats(2, 2), feats(2, 2), tau=1.0 / 32.0)
    ops.info_nce(feats(2, 2), feats(2, 2), tau=1024)
    assert [c[1]["tau"] for c in lib.exports()] == [1.0 / 32.0, 1024.0]


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (7, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    before = ops.last_stats
    with pytest.raises(exc, match=f"status {status}"):
        ops.info_nce(feats(4, 2), feats(4, 2))
    assert ops.last_stats is before


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.info_nce(feats(4, 2), feats(4, 2))
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_infonce")
    assert names[i:i + 4] == ["rlap_infonce", "rlap_workspace_needed", "rlap_set_workspace", "rlap_infonce"]
    assert lib.calls[i + 2][1]["ws_bytes"] >= 1 << 20


@pytest.mark.parametrize("which", ["both", "anchor", "sample"])
def test_autograd_calls_the_backward_export_once(lib, which):
    a = feats(4, 3).requires_grad_(which in ("both", "anchor"))
    b = feats(4, 3, 0.25).requires_grad_(which in ("both", "sample"))
    loss = ops.info_nce(a, b, tau=0.5, positive="raw")
    assert loss.requires_grad
    (2.5 * loss).backward()
    (fname, f), (bname, c) = lib.exports()
    assert (fname, bname) == ("rlap_infonce", "rlap_infonce_backward")
    assert (c["n"], c["F"], c["tau"], c["flags"]) == (4, 3, 0.5, 1) == (f["n"], f["F"], f["tau"], f["flags"])
    assert c["a"] == a.detach().reshape(-1).tolist() and c["b"] == b.detach().reshape(-1).tolist()
    assert c["z"] == [2.0] * 4 and c["g"] == [2.5]                  # the forward's row sums; the upstream gradient, on the device
    if a.requires_grad:
        assert a.grad.shape == a.shape and a.grad.dtype == torch.float32 and bool((a.grad == 3).all())
    else:
        assert a.grad is None
    if b.requires_grad:
        assert bool((b.grad == 4).all())
    else:
        assert b.grad is None
    assert ops.last_stats["rows"] == 4 and ops.last_stats["host_syncs"] == 0


def test_rows_are_not_differentiable(lib):
    a = feats(4, 3).requires_grad_(True)
    loss, rows = ops.info_nce(a, feats(4, 3), return_rows=True)
    assert loss.requires_grad and not rows.requires_grad


def test_no_graph_is_recorded_without_requires_grad(lib):
    assert not ops.info_nce(feats(4, 3), feats(4, 3)).requires_grad
    a = feats(4, 3).requires_grad_(True)
    with torch.no_grad():
        assert not ops.info_nce(a, a).requires_grad
    assert [c[0] for c in lib.exports()] == ["rlap_infonce"] * 2


def test_infonce_info_layout(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_infonce_info", "InfonceInfo")
    assert [f for f, _ in _lib.InfonceInfo._fields_] == ["rows", "features", "parts", "arena_bytes", "host_syncs", "pad"]


def test_exports_and_flags_are_declared():
    assert {"rlap_infonce", "rlap_infonce_backward"} <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "enum { RLAP_INFONCE_POSITIVE_RAW = 1 };" in hdr
    assert "not finite" in hdr[hdr.index("The fused InfoNCE"):hdr.index("enum { RLAP_INFONCE_POSITIVE_RAW")]


# ------------------------------------------------------------------------------------------------ the adapter
def test_node_contrast_makes_two_calls_with_the_roles_swapped(lib):
    h1, h2 = feats(4, 3).requires_grad_(True), feats(4, 3, 0.5).requires_grad_(True)
    loss = adapters.NodeContrast(tau=0.5)(h1, h2)
    assert float(loss.detach()) == 1.5 and loss.dtype == torch.float64            # 0.5 * (1.5 + 1.5)
    x, y = lib.exports()
    assert x[0] == y[0] == "rlap_infonce" and x[1]["flags"] == y[1]["flags"] == 1 and x[1]["tau"] == 0.5    # "raw" by default
    assert x[1]["a"] == y[1]["b"] == h1.detach().reshape(-1).tolist() and x[1]["b"] == y[1]["a"] == h2.detach().reshape(-1).tolist()
    loss.backward()
    back = [c for c in lib.exports() if c[0] == "rlap_infonce_backward"]
    assert len(back) == 2 and sorted(c[1]["g"] for c in back) == [[0.5], [0.5]]
    assert bool((h1.grad == 3 + 4).all()) and bool((h2.grad == 4 + 3).all())       # (the stub's gradients do not scale with g)


def test_node_contrast_takes_the_views_of_a_layer(lib):
    h = torch.stack([feats(4, 3), feats(4, 3, 0.5), feats(4, 3, 9.0)])
    adapters.NodeContrast(tau=0.4, positive="scaled")(h)
    x, y = lib.exports()
    assert x[1]["a"] == h[0].reshape(-1).tolist() and x[1]["b"] == h[1].reshape(-1).tolist() and x[1]["flags"] == 0
    assert y[1]["a"] == h[1].reshape(-1).tolist() and y[1]["b"] == h[0].reshape(-1).tolist()
    for bad in (feats(4, 3), h[:1]):
        with pytest.raises(ValueError):
            adapters.NodeContrast()(bad)
