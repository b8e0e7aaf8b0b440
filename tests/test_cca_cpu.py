"""The fused CCA-SSG loss (ops.cca_loss, rlap_cca_loss / rlap_cca_loss_backward) without a GPU:

  * the rule -- the host mirror (tests/csrc/cca_mirror.cc, every value from rlap_amd/csrc/rlap_cca.h, contraction off) against a
    float64 torch restatement of CCA-SSG/model.py:77-78 and CCA-SSG/main.py:111-124 and their autograd, for lambd in {0, 1e-3, 1};
    the order's invariances; the special cases;
  * the index arithmetic of the header in a stand-alone program under -fsanitize=address,undefined, exhaustively for N <= 300;
  * the Python -> C mapping of both exports on a stub library, the layout of rlap_cca_info, adapters.CCAContrast and
    adapters.drop_feature.

The bounds of the first group are four times the largest differences measured with these inputs (DESIGN 4.16 has the figures): the
rule's error is that of float32 standardised values and of float32 chains, a property of the formats and not of the seed.  Measured
here: loss 4.09e-8 relative (N = 33, F = 3, lambd = 1), gradients 1.50e-6 of the largest entry (N = 129, F = 512, lambd = 1, where
the decorrelation term, which passes through the float32 residuals and a float32 chain of length 512, carries the gradient);
dec1 / dec2 1.32e-7 and inv 3.42e-8 relative to the term itself.  Every term is checked on its own, because the loss can cancel:
at (N, F) = (2, 1) the standardised values are +-1/sqrt(2) whatever h is, so inv = -0.5, dec1 = dec2 = 0.25, the loss at lambd = 1 is
0 up to rounding and every gradient is exactly zero.  There the loss is bounded relative to |inv| + lambd (dec1 + dec2) (measured
7.67e-8 of it, held to the same bound as the others) and the gradients relative to g / (N sd), the size of the terms that cancel in
dh (measured 7.26e-8 of it).
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import cca_mirror as cm
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, f64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_BOUND = 4 * 4.09e-8     # relative to the loss (or to the sum of its terms' sizes where it cancels)
GRAD_BOUND = 4 * 1.50e-6     # relative to the largest gradient entry
DEC_BOUND = 4 * 1.32e-7      # |dec - reference|, relative to dec itself (a sum of squares: nothing cancels)
INV_BOUND = 4 * 3.42e-8      # |inv - reference|, relative to |inv|
G_UP = 0.75


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return cm.build(tmp_path_factory.mktemp("cca"))


# ------------------------------------------------------------------------------------------------ the rule
SHAPES = [(2, 1), (33, 3), (65, 33), (300, 100), (129, 512), (2708, 64)]


@pytest.mark.parametrize("lambd", [0.0, 1e-3, 1.0])
@pytest.mark.parametrize("n,f", SHAPES)
def test_mirror_against_the_float64_restatement(mirror, n, f, lambd):
    a, b = cm.views(n, f, 1000 + n)
    m = cm.run(mirror, a, b, lambd, g=G_UP)
    terms, ga, gb = cm.restatement(a, b, lambd, g=G_UP)
    loss, inv, dec1, dec2 = terms
    size = abs(inv) + lambd * (dec1 + dec2)
    cancels = abs(loss) < 0.05 * size
    rel = abs(m["loss"] - loss) / (size if cancels else abs(loss))
    gmax = max(np.abs(ga).max(), np.abs(gb).max())
    sd_min = min(m["colstat"][f:2 * f].min(), m["colstat"][3 * f:].min())
    gscale = G_UP / (n * sd_min) if n == 2 else gmax          # (N = 2: every gradient is zero, see the top)
    grel = max(np.abs(m["ga"] - ga).max(), np.abs(m["gb"] - gb).max()) / gscale
    drel = max(abs(m["dec1"] - dec1) / dec1, abs(m["dec2"] - dec2) / dec2)
    irel = abs(m["inv"] - inv) / abs(inv)
    print(f"n={n} F={f} lambd={lambd}: loss {loss:.6g} rel {rel:.3g}{' (cancels)' if cancels else ''}, gradients rel {grel:.3g}, "
          f"dec rel {drel:.3g} (abs {max(abs(m['dec1'] - dec1), abs(m['dec2'] - dec2)):.3g}), inv rel {irel:.3g} (abs {abs(m['inv'] - inv):.3g})")
    assert cancels == ((n, f, lambd) == (2, 1, 1.0))
    assert rel <= LOSS_BOUND
    assert grel <= GRAD_BOUND
    assert abs(m["dec1"] - dec1) <= DEC_BOUND * dec1 and abs(m["dec2"] - dec2) <= DEC_BOUND * dec2
    assert abs(m["inv"] - inv) <= INV_BOUND * abs(inv)


def test_column_statistics_against_numpy(mirror):
    a, b = cm.views(300, 20, 3)
    m = cm.run(mirror, a, b, 1e-3)
    for v, x in enumerate((a, b)):
        x = x.astype(np.float64)
        assert np.abs(m["colstat"][40 * v:40 * v + 20] - x.mean(0)).max() <= 1e-14
        assert np.abs(m["colstat"][40 * v + 20:40 * v + 40] - x.std(0, ddof=1)).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ order and invariance
@pytest.mark.parametrize("n,f", [(65, 33), (300, 20)])
def test_threads_and_tiling_change_no_bit(mirror, n, f):
    """The mirror computes every Gram entry and every row of P on its own, so `block` and `threads` only change how they are
    grouped and dealt out: this pins the mirror, not the kernels.  The guard against an order that depends on the grid is the
    bit-for-bit comparison on the device (tests/test_gpu_cca.py: several parts, several workgroups per view)."""
    a, b = cm.views(n, f, 7)
    base = cm.run(mirror, a, b, 1e-3, g=1.0, block=32, threads=8)
    for block, threads in ((1, 8), (7, 3), (128, 1), (1000, 8)):
        other = cm.run(mirror, a, b, 1e-3, g=1.0, block=block, threads=threads)
        for key in ("terms", "colstat", "gram", "ga", "gb"):
            assert np.asarray(base[key]).tobytes() == np.asarray(other[key]).tobytes(), (block, threads, key)


def test_parts_depend_on_n_and_f_alone(mirror):
    for n in (2, 32, 33, 300, 2708, 34493, 169343):
        for f in (1, 64, 100, 512):
            p = mirror.cca_parts(n, f)
            tiles = (n + 31) // 32
            assert 1 <= p <= min(tiles, 64) and mirror.cca_part_begin(n, f, 0) == 0 and mirror.cca_part_begin(n, f, p) == 32 * tiles
            assert all(mirror.cca_part_begin(n, f, q) % 32 == 0 for q in range(p + 1))
    assert mirror.cca_parts(2708, 64) == 64 and mirror.cca_parts(300, 512) == 10 and mirror.cca_parts(169343, 512) == 29
    assert [mirror.cca_pair_groups(f) for f in (1, 64, 65, 128, 256, 512)] == [1, 1, 1, 1, 3, 9]


@pytest.mark.parametrize("f", [3, 32, 33])
def test_zero_columns_behind_the_padded_image_change_no_bit(mirror, f):
    """Zero columns behind F enter the Gram sums of no result and the backward chain as fmaf(0, 0, acc) steps.  (Zero columns in
    the INPUT are another matter: they have zero variance.)"""
    a, b = cm.views(65, f, 11)
    m = cm.run(mirror, a, b, 1e-3, g=1.0)
    for pad in (1, 3):
        w = cm.run(mirror, a, b, 1e-3, g=1.0, pad_tiles=pad)
        for key in ("terms", "colstat", "gram", "ga", "gb"):
            assert np.asarray(m[key]).tobytes() == np.asarray(w[key]).tobytes(), (pad, key)


def test_the_residuals_are_exactly_symmetric(mirror):
    a, b = cm.views(129, 40, 13)
    m = cm.run(mirror, a, b, 1e-3)
    for v in range(2):
        assert m["gram"][v].tobytes() == np.ascontiguousarray(m["gram"][v].T).tobytes()
        assert np.abs(np.diag(m["gram"][v]) - 1.0 / 129).max() < 1e-6       # c_kk = (N - 1) / N: the deviation is the unbiased one


def test_lambd_zero_is_the_invariance_term_alone(mirror):
    n, f = 65, 33
    a, b = cm.views(n, f, 17)
    m = cm.run(mirror, a, b, 0.0, g=G_UP)
    assert m["terms"][0].tobytes() == m["terms"][1].tobytes()                # loss == inv
    # the backward pass of dz = g * (-z_other / N) alone, through the standardisation, in float64 numpy
    mean = [m["colstat"][0:f], m["colstat"][2 * f:3 * f]]
    sd = [m["colstat"][f:2 * f], m["colstat"][3 * f:]]
    z = [((x.astype(np.float64) - mean[v]) / sd[v]).astype(np.float32).astype(np.float64) for v, x in enumerate((a, b))]
    for v, key in ((0, "ga"), (1, "gb")):
        dz = G_UP * (-z[1 - v] / n)
        want = (dz - dz.mean(0) - z[v] * (dz * z[v]).sum(0) / (n - 1)) / sd[v]
        assert np.abs(m[key] - want).max() <= 2.0 ** -23 * np.abs(want).max()   # one float32 rounding of the result
    big = cm.run(mirror, a, b, 1.0, g=G_UP)
    assert big["ga"].tobytes() != m["ga"].tobytes() and big["terms"][1].tobytes() == m["terms"][1].tobytes()


def test_a_constant_column_gives_nan_in_the_mirror_and_in_the_restatement(mirror):
    a, b = cm.views(40, 5, 19)
    a[:, 2] = 1.5
    m = cm.run(mirror, a, b, 1e-3, g=1.0)
    terms, ga, _ = cm.restatement(a, b, 1e-3)
    assert math.isnan(m["loss"]) and math.isnan(terms[0])
    assert m["colstat"][5 + 2] == 0.0 and np.isnan(m["ga"][:, 2]).all() and np.isnan(ga[:, 2]).all()


def test_lambd_range(mirror):
    assert all(mirror.cca_lambd_ok(x) for x in (0.0, 1e-3, 1.0, 1e300))
    assert not any(mirror.cca_lambd_ok(x) for x in (-1e-9, -1.0, float("nan"), float("inf")))


# ------------------------------------------------------------------------------------------------ the index arithmetic, under the sanitizers
def test_the_index_arithmetic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "cca_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "cca_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "300 sizes, 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_cca_loss": "h a b n F lambd flags terms colstat gram info",
    "rlap_cca_loss_backward": "h a b n F lambd flags colstat gram g ga gb info",
}
ARENA = 9876
TERMS = [1.5, -2.0, 3.0, 4.0]


def f32_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


class CcaStub(StubLib):
    """Records both exports; the forward writes terms = 1.5, -2, 3, 4, colstat = 0.5 and gram = 0.25; the backward ga = 3, gb = 4."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        status = self.statuses.pop(0) if self.statuses else self.status
        n, F = a["n"], a["F"]
        rec = {k: a[k] for k in ("n", "F", "lambd", "flags")}
        rec["a"], rec["b"] = f32_at(a["a"], n * F), f32_at(a["b"], n * F)
        back = name.endswith("backward")
        if back:
            rec["colstat"], rec["gram"], rec["g"] = f64_at(a["colstat"], 4 * F), f32_at(a["gram"], 2 * F * F), f64_at(a["g"], 1)
        self.calls.append((name, rec))
        if status:
            return status
        if back:
            for key, v in (("ga", 3.0), ("gb", 4.0)):
                out = ctypes.cast(a[key], ctypes.POINTER(ctypes.c_float))
                for i in range(n * F):
                    out[i] = v
        else:
            assert a["colstat"] == a["terms"] + 32                        # one buffer: terms | colstat
            out = ctypes.cast(a["terms"], ctypes.POINTER(ctypes.c_double))
            for i, v in enumerate(TERMS + [0.5] * (4 * F)):
                out[i] = v
            out = ctypes.cast(a["gram"], ctypes.POINTER(ctypes.c_float))
            for i in range(2 * F * F):
                out[i] = 0.25
        info = a["info"]._obj
        info.rows, info.features, info.parts, info.arena_bytes, info.host_syncs = n, F, 7, ARENA, 0
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, CcaStub())


def feats(n, f, shift=0.0):
    return (torch.arange(n * f, dtype=torch.float32).reshape(n, f) / 4.0 - 1.0 + shift)


def test_arguments_of_the_forward_export(lib):
    a, b = feats(5, 3), feats(5, 3, 0.5)
    out = ops.cca_loss(a, b, lambd=0.5, return_terms=True)
    (name, c), = lib.exports()
    assert name == "rlap_cca_loss"
    assert (c["n"], c["F"], c["lambd"], c["flags"]) == (5, 3, 0.5, 0)
    assert c["a"] == a.reshape(-1).tolist() and c["b"] == b.reshape(-1).tolist()
    assert len(out) == 4 and all(t.dim() == 0 and t.dtype == torch.float64 for t in out) and [float(t) for t in out] == TERMS
    assert ops.last_stats == {"rows": 5, "features": 3, "parts": 7, "arena_bytes": ARENA, "host_syncs": 0}
    assert not out[0].requires_grad


def test_defaults(lib):
    out = ops.cca_loss(feats(2, 2), feats(2, 2))
    (_, c), = lib.exports()
    assert (c["lambd"], c["flags"]) == (1e-3, 0) and isinstance(out, torch.Tensor) and out.dim() == 0 and float(out) == 1.5


def test_non_contiguous_inputs_are_packed(lib):
    a = feats(3, 5).t()          # (5, 3), strided
    ops.cca_loss(a, a, lambd=1.0)
    (_, c), = lib.exports()
    assert c["a"] == a.contiguous().reshape(-1).tolist() and (c["n"], c["F"]) == (5, 3)


BAD = [
    (torch.zeros(5), torch.zeros(5), 1e-3),                                    # not 2-D
    (torch.zeros(1, 5, 3), torch.zeros(1, 5, 3), 1e-3),
    (torch.zeros(5, 3), torch.zeros(5, 4), 1e-3),                              # shapes differ
    (torch.zeros(5, 3), torch.zeros(4, 3), 1e-3),
    (torch.zeros(5, 3, dtype=torch.float64), torch.zeros(5, 3, dtype=torch.float64), 1e-3),   # not float32
    (torch.zeros(5, 3), torch.zeros(5, 3, dtype=torch.float16), 1e-3),
    (torch.zeros(5, 3, dtype=torch.int64), torch.zeros(5, 3, dtype=torch.int64), 1e-3),
    ([[1.0, 2.0], [3.0, 4.0]], torch.zeros(2, 2), 1e-3),                       # not a tensor
    (torch.zeros(5, 3), torch.zeros(5, 3, device="meta"), 1e-3),               # two devices
    (torch.zeros(0, 3), torch.zeros(0, 3), 1e-3),                              # N < 2
    (torch.zeros(1, 3), torch.zeros(1, 3), 1e-3),
    (torch.zeros(5, 0), torch.zeros(5, 0), 1e-3),                              # no column
    (torch.zeros(2, 513), torch.zeros(2, 513), 1e-3),                          # F > 512
    (torch.zeros(5, 3), torch.zeros(5, 3), -1e-3),                             # lambd negative or not finite
    (torch.zeros(5, 3), torch.zeros(5, 3), float("nan")),
    (torch.zeros(5, 3), torch.zeros(5, 3), float("inf")),
    (torch.zeros(5, 3), torch.zeros(5, 3), "1e-3"),
    (torch.zeros(5, 3), torch.zeros(5, 3), True),
    (torch.zeros(5, 3), torch.zeros(5, 3), None),
]


@pytest.mark.parametrize("a,b,lambd", BAD)
def test_bad_arguments_raise_value_error_before_any_call(lib, monkeypatch, a, b, lambd):
    def reached(*args, **kw):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    with pytest.raises(ValueError):
        ops.cca_loss(a, b, lambd=lambd)
    assert lib.exports() == []


def test_the_ends_of_the_ranges_are_inside(lib):
    ops.cca_loss(feats(2, 512), feats(2, 512), lambd=0)
    (_, c), = lib.exports()
    assert (c["n"], c["F"], c["lambd"]) == (2, 512, 0.0)


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (7, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    before = ops.last_stats
    with pytest.raises(exc, match=f"status {status}"):
        ops.cca_loss(feats(4, 2), feats(4, 2))
    assert ops.last_stats is before


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.cca_loss(feats(4, 2), feats(4, 2))
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_cca_loss")
    assert names[i:i + 4] == ["rlap_cca_loss", "rlap_workspace_needed", "rlap_set_workspace", "rlap_cca_loss"]
    assert lib.calls[i + 2][1]["ws_bytes"] >= 1 << 20


@pytest.mark.parametrize("which", ["both", "first", "second"])
def test_autograd_calls_the_backward_export_once(lib, which):
    a = feats(4, 3).requires_grad_(which in ("both", "first"))
    b = feats(4, 3, 0.25).requires_grad_(which in ("both", "second"))
    loss = ops.cca_loss(a, b, lambd=0.5)
    assert loss.requires_grad
    (2.5 * loss).backward()
    (fname, f), (bname, c) = lib.exports()
    assert (fname, bname) == ("rlap_cca_loss", "rlap_cca_loss_backward")
    assert (c["n"], c["F"], c["lambd"], c["flags"]) == (4, 3, 0.5, 0) == (f["n"], f["F"], f["lambd"], f["flags"])
    assert c["a"] == a.detach().reshape(-1).tolist() and c["b"] == b.detach().reshape(-1).tolist()
    assert c["colstat"] == [0.5] * 12 and c["gram"] == [0.25] * 18 and c["g"] == [2.5]   # the forward's; the upstream gradient, on the device
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
    loss, inv, dec1, dec2 = ops.cca_loss(a, feats(4, 3), return_terms=True)
    assert loss.requires_grad and not (inv.requires_grad or dec1.requires_grad or dec2.requires_grad)
    assert [float(t.detach()) for t in (loss, inv, dec1, dec2)] == TERMS


def test_no_graph_is_recorded_without_requires_grad(lib):
    assert not ops.cca_loss(feats(4, 3), feats(4, 3)).requires_grad
    a = feats(4, 3).requires_grad_(True)
    with torch.no_grad():
        assert not ops.cca_loss(a, a).requires_grad
    assert [c[0] for c in lib.exports()] == ["rlap_cca_loss"] * 2


def test_flags_are_reserved(lib):
    """ops always passes 0; the library answers anything else with RLAP_E_BAD_ARG (tests/test_gpu_cca_cabi.py), which ops raises as
    a ValueError."""
    lib.status = 3
    with pytest.raises(ValueError):
        ops.cca_loss(feats(4, 2), feats(4, 2))
    assert lib.exports()[0][1]["flags"] == 0
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    doc = hdr[hdr.index("The fused CCA-SSG loss"):hdr.index("} rlap_cca_info;")]
    assert "reserved, 0" in doc and "zero variance" in doc
    api = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_api.hip")).read()
    assert "flags != 0" in api[api.index("int cca_check("):api.index("int rlap_cca_loss(")]


def test_cca_info_layout(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_cca_info", "CcaInfo")
    assert [f for f, _ in _lib.CcaInfo._fields_] == ["rows", "features", "parts", "arena_bytes", "host_syncs", "pad"]


def test_exports_are_declared():
    assert {"rlap_cca_loss", "rlap_cca_loss_backward"} <= set(_lib.EXPORTS)


# ------------------------------------------------------------------------------------------------ the adapters
def test_cca_contrast_takes_two_embeddings(lib):
    h1, h2 = feats(4, 3).requires_grad_(True), feats(4, 3, 0.5).requires_grad_(True)
    loss = adapters.CCAContrast(lambd=0.5)(h1, h2)
    assert float(loss.detach()) == 1.5 and loss.dtype == torch.float64 and loss.dim() == 0
    (_, c), = lib.exports()
    assert c["lambd"] == 0.5 and c["a"] == h1.detach().reshape(-1).tolist() and c["b"] == h2.detach().reshape(-1).tolist()
    loss.backward()
    assert bool((h1.grad == 3).all()) and bool((h2.grad == 4).all())
    assert adapters.CCAContrast().lambd == 1e-3


def test_cca_contrast_takes_the_views_of_a_layer(lib):
    h = torch.stack([feats(4, 3), feats(4, 3, 0.5), feats(4, 3, 9.0)])
    adapters.CCAContrast()(h)
    (_, c), = lib.exports()
    assert c["a"] == h[0].reshape(-1).tolist() and c["b"] == h[1].reshape(-1).tolist() and c["lambd"] == 1e-3
    for bad in (feats(4, 3), h[:1]):
        with pytest.raises(ValueError):
            adapters.CCAContrast()(bad)


def reference_drop_feature(x, drop_prob, generator):
    """CCA-SSG/aug.py's three lines, the uniforms from a generator."""
    drop_mask = torch.empty((x.size(1),), dtype=torch.float32, device=x.device).uniform_(0, 1, generator=generator) < drop_prob
    x = x.clone()
    x[:, drop_mask] = 0
    return x, drop_mask


@pytest.mark.parametrize("p", [0.0, 0.3, 1.0])
def test_drop_feature_against_the_reference_lines(p):
    x = feats(7, 40, 100.0)                                              # no zero among the inputs
    out = adapters.drop_feature(x, p, views=3, generator=torch.Generator().manual_seed(5))
    assert out.shape == (3, 7, 40) and out.dtype == x.dtype
    gen = torch.Generator().manual_seed(5)
    masks = []
    for v in range(3):
        want, mask = reference_drop_feature(x, p, gen)
        masks.append(mask)
        assert torch.equal(out[v], want)
        assert bool((out[v][:, mask] == 0).all()) and torch.equal(out[v][:, ~mask], x[:, ~mask])
    if p == 0.3:
        assert 0 < int(masks[0].sum()) < 40 and not torch.equal(masks[0], masks[1])     # one mask per view
    assert torch.equal(x, feats(7, 40, 100.0))                           # the input is left as it was
    assert adapters.drop_feature(x, 0.5).shape == (1, 7, 40)
    for bad in ((x[0], 0.5, 1), (x, 1.5, 1), (x, -0.1, 1), (x, 0.5, 0), (x, "0.5", 1)):
        with pytest.raises(ValueError):
            adapters.drop_feature(bad[0], bad[1], views=bad[2])
