"""The per-view batch norm with fused activations (ops.batch_norm, rlap_batch_norm / rlap_batch_norm_backward) without
a GPU:

  * the rule -- the host mirror (tests/csrc/norm_mirror.cc, every value from rlap_amd/csrc/rlap_norm.h, contraction off) against
    torch.nn.functional.batch_norm per layer in float64, relu in front and relu / prelu behind as flagged: training and evaluation,
    every pre x post, both slope forms, with and without affine parameters; the running buffers after three layers against three
    sequential torch calls; the gradients against float64 autograd; the chunk rule restated in numpy, bit for bit;
  * the map functions and the mirror's loops in a stand-alone program under -fsanitize=address,undefined;
  * the Python -> C mapping of both exports on a stub library, every refusal, the layout of rlap_norm_info, the module.

Bounds.  Forward: |y - y64| <= 2^-24 |y64| + 1e-13 (|xh w| + |b|) -- the one rounding to float32, and the float64 rounding of two
differently ordered float64 evaluations.  Gradients: half a float32 unit in the last place of the reference plus GRAD_K times the
sum of the magnitudes of the gradient's terms (gx: rstd w gv, rstd w A / N, rstd w xh B / N; the parameter gradients: their N L
summands); GRAD_K is four times the largest ratio measured with these inputs (mirror against torch float64, on the CPU: 4.95e-14,
at (L, N, F) = (2, 1000, 8) in training mode; 2.72e-15 at (3, 257, 16), 3.6e-17 at (1, 2, 8), none above the half unit elsewhere
and in evaluation mode), and stays under the cap of 1e-10.  The margin is there because the two sides sum N terms in different
orders.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import norm_mirror as nm
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, f64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_F64 = 1e-13
GRAD_K_MEASURED = 4.95e-14
GRAD_K = 4 * GRAD_K_MEASURED
assert GRAD_K <= 1e-10
SHAPES = [(1, 2, 8), (3, 257, 16), (2, 513, 11), (3, 100, 33), (2, 1000, 8)]
POSTS = [("none", False), ("relu", False), ("prelu", False), ("prelu", True)]


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return nm.build(tmp_path_factory.mktemp("norm"))


def half_ulp32(ref):
    return 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def case(d, f, pre, post, per_channel, affine, training):
    """The keyword arguments of the mirror and of the restatement for one combination."""
    slope = None if post != "prelu" else (d["slope"] if per_channel else d["slope"][:1])
    common = {"weight": d["weight"] if affine else None, "bias": d["bias"] if affine else None, "slope": slope,
              "running_mean": None if training else d["running_mean"], "running_var": None if training else d["running_var"]}
    return common, nm.flags_of(pre, post, per_channel and post == "prelu", training)


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("L,n,f", SHAPES)
def test_mirror_forward_against_torch_float64(mirror, L, n, f, training):
    d = nm.inputs(L, n, f, 100 + n)
    worst = 0.0
    for pre in ("none", "relu"):
        for post, per_channel in POSTS:
            for affine in (True, False):
                kw, flags = case(d, f, pre, post, per_channel, affine, training)
                m = nm.forward(mirror, d["x"], flags=flags, **kw)
                r = nm.restatement(d["x"], training=training, pre=pre, post=post, **kw)
                w = np.abs(d["weight"].astype(np.float64)) if affine else 1.0
                b = np.abs(d["bias"].astype(np.float64)) if affine else 0.0
                bound = 2.0 ** -24 * np.abs(r["y"]) + FWD_F64 * (np.abs(r["xh"]) * w + b)
                err = np.abs(m["y"].astype(np.float64) - r["y"])
                worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
                assert (err <= bound).all(), (pre, post, per_channel, affine, float((err / np.maximum(bound, 1e-300)).max()))
                assert np.isfinite(m["y"]).all()
    print(f"L={L} n={n} F={f} training={training}: largest |y - y64| / bound {worst:.3g}")


@pytest.mark.parametrize("pre", ["none", "relu"])
@pytest.mark.parametrize("n,f", [(2, 8), (257, 16), (1000, 9)])
def test_running_buffers_after_three_layers(mirror, n, f, pre):
    """Against three sequential torch calls in float64, like everything else here, on float32 buffers: each call's update is rounded
    to float32, as a float32 module stores it (norm_mirror.torch_buffers).  A float32 torch call is no reference for one unit in
    the last place: it rounds the batch mean to float32 before the update, which in a column whose means cancel costs it tens of
    units (24 measured at (N, F) = (257, 16))."""
    d = nm.inputs(3, n, f, 7 + n)
    m = nm.forward(mirror, d["x"], running_mean=d["running_mean"], running_var=d["running_var"], momentum=0.1, flags=nm.flags_of(pre))
    rm, rv = nm.torch_buffers(d["x"], d["running_mean"], d["running_var"], 0.1, 1e-5, pre)
    assert (np.abs(m["running_mean"] - rm) <= np.spacing(np.abs(rm))).all()
    assert (np.abs(m["running_var"] - rv) <= np.spacing(np.abs(rv))).all()
    assert not np.array_equal(m["running_mean"], d["running_mean"])
    # the layers in order: layer by layer through the (N, F) call gives the same bits
    rm1, rv1 = d["running_mean"], d["running_var"]
    for l in range(3):
        one = nm.forward(mirror, d["x"][l:l + 1], running_mean=rm1, running_var=rv1, momentum=0.1, flags=nm.flags_of(pre))
        rm1, rv1 = one["running_mean"], one["running_var"]
        assert one["y"].tobytes() == m["y"][l:l + 1].tobytes() and one["stat"].tobytes() == m["stat"][l:l + 1].tobytes()
    assert rm1.tobytes() == m["running_mean"].tobytes() and rv1.tobytes() == m["running_var"].tobytes()


def grad_terms(d, r, kw, flags, training, eps=1e-5):
    """Per element the sum of the magnitudes of gx's three terms, and per column those of the parameter gradients' summands, from
    float64 numpy on the restatement's xh."""
    x, gy, xh = d["x"].astype(np.float64), d["gy"].astype(np.float64), r["xh"]
    w = kw["weight"].astype(np.float64) if kw["weight"] is not None else np.ones(x.shape[-1])
    b = kw["bias"].astype(np.float64) if kw["bias"] is not None else np.zeros(x.shape[-1])
    u = np.maximum(x, 0.0) if flags & nm.PRE_RELU else x
    rstd = 1.0 / np.sqrt(u.var(1, keepdims=True) + eps) if training else 1.0 / np.sqrt(kw["running_var"].astype(np.float64) + eps)
    v = xh * w + b
    a = kw["slope"].astype(np.float64) if kw["slope"] is not None else 0.0
    dpost = np.where(v > 0, 1.0, a if flags & nm.POST_PRELU else 0.0) if flags & (nm.POST_RELU | nm.POST_PRELU) else np.ones_like(v)
    gv = gy * dpost
    n = x.shape[1]
    sw = np.abs(rstd * w)
    t = sw * np.abs(gv)
    if training:
        t = t + sw * np.abs(gv.sum(1, keepdims=True)) / n + sw * np.abs(xh) * np.abs((gv * xh).sum(1, keepdims=True)) / n
    return {"gx": t, "gweight": np.abs(gv * xh).sum((0, 1)), "gbias": np.abs(gv).sum((0, 1)),
            "gslope": np.abs(gy * v * (v <= 0)).sum((0, 1))}


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("L,n,f", SHAPES)
def test_mirror_gradients_against_float64_autograd(mirror, L, n, f, training):
    d = nm.inputs(L, n, f, 200 + n)
    worst = 0.0
    for pre in ("none", "relu"):
        for post, per_channel in POSTS:
            for affine in (True, False):
                kw, flags = case(d, f, pre, post, per_channel, affine, training)
                fw = nm.forward(mirror, d["x"], flags=flags, **kw)
                m = nm.backward(mirror, d["x"], d["gy"], fw["stat"], flags=flags, **kw)
                r = nm.restatement(d["x"], gy=d["gy"], training=training, pre=pre, post=post, **kw)
                terms = grad_terms(d, r, kw, flags, training)
                if post == "prelu" and not per_channel:
                    terms["gslope"] = terms["gslope"].sum(keepdims=True)
                for key in ("gx", "gweight", "gbias", "gslope"):
                    if r.get(key) is None:
                        continue
                    ref = r[key]
                    excess = np.abs(m[key].astype(np.float64) - ref) - half_ulp32(ref)
                    ratio = float((excess / np.maximum(terms[key], 1e-300)).max())
                    worst = max(worst, ratio)
                    assert (excess <= GRAD_K * terms[key]).all(), (key, pre, post, per_channel, affine, ratio)
    print(f"L={L} n={n} F={f} training={training}: largest float64 term ratio {worst:.3g} (bound {GRAD_K:.3g})")


# ------------------------------------------------------------------------------------------------ the chunk rule, restated
def chunk_rule(terms):
    total = np.float64(0.0)
    for b in range(0, len(terms), 256):
        c = np.float64(0.0)
        for t in terms[b:b + 256]:
            c = c + t
        total = total + c
    return total


@pytest.mark.parametrize("n", [2, 255, 256, 257, 513])
def test_the_chunk_rule_restated_in_numpy(mirror, n):
    d = nm.inputs(1, n, 8, n)
    m = nm.forward(mirror, d["x"], weight=d["weight"], bias=d["bias"], flags=nm.PRE_RELU)
    x = d["x"][0].astype(np.float64)
    for k in range(8):
        u = np.where(d["x"][0, :, k] > 0, x[:, k], 0.0)
        dd = u - u[0]
        mm = chunk_rule(dd) / np.float64(n)
        var = max(chunk_rule(dd * dd) / np.float64(n) - mm * mm, 0.0)
        rstd = np.float64(1.0) / np.sqrt(var + np.float64(1e-5))
        y = (((dd - mm) * rstd) * np.float64(d["weight"][k]) + np.float64(d["bias"][k])).astype(np.float32)
        assert np.array([u[0], mm, rstd]).tobytes() == m["stat"][0, :, k].tobytes(), k
        assert y.tobytes() == np.ascontiguousarray(m["y"][0, :, k]).tobytes(), k


def test_a_column_of_zero_variance_gives_no_nan(mirror):
    d = nm.inputs(2, 40, 8, 3)
    m = nm.forward(mirror, d["x"], flags=nm.PRE_RELU)
    for k in (1, 2):   # the constant column; the column the relu empties
        assert (m["stat"][:, 1, k] == 0).all() and (m["stat"][:, 2, k] == 1.0 / np.sqrt(1e-5)).all() and (m["y"][:, :, k] == 0).all()


# ------------------------------------------------------------------------------------------------ the map, under the sanitizers
def test_the_map_functions_and_the_loops_under_asan_ubsan(tmp_path):
    exe = tmp_path / "norm_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "norm_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "600"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " sizes, 0 failures" in r.stdout


def test_constants_and_dispatch(mirror):
    c = nm.constants(mirror)
    assert c["chunk"] == 256 and c["max_f"] == _lib.NORM_MAX_F == ops.NORM_MAX_F == 4096
    src = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_norm.hip")).read()
    assert "NM_MAX_GRID = norm::MAX_GRID" in src and "NM_WAVES = norm::GROUP_WAVES" in src     # the launchers read the header's
    assert nm.dispatch(mirror, 64, True) == {"vec": True, "lanes": 16, "lg": 4, "ftiles": 1}
    assert nm.dispatch(mirror, 64, False) == {"vec": False, "lanes": 64, "lg": 6, "ftiles": 1}
    assert nm.dispatch(mirror, 516, True)["ftiles"] == 3 and nm.dispatch(mirror, 33, True)["vec"] is False
    assert mirror.norm_forward_bytes(3, 513, 33, 0) == (2 * 3 * 3 * 33 * 8 + 255) // 256 * 256 + (2 * 3 * 33 * 8 + 255) // 256 * 256
    assert mirror.norm_forward_bytes(3, 513, 33, nm.EVAL) == 0


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_batch_norm": "h x L N F weight bias slope rm rv momentum eps flags y stat info",
    "rlap_batch_norm_backward": "h x gy L N F weight bias slope rm rv eps flags stat gx gweight gbias gslope info",
}
ARENA = 4321


def f32_at(addr, count):
    return None if addr is None else list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


def fill(addr, count, value, ctype=ctypes.c_float):
    if addr is not None:
        out = ctypes.cast(addr, ctypes.POINTER(ctype))
        for i in range(count):
            out[i] = value


class NormStub(StubLib):
    """Records both exports; the forward writes y = 2, stat = 0.5 and adds 1 to the running buffers; the backward gx = 3,
    gweight = 4, gbias = 5, gslope = 6."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        status = self.statuses.pop(0) if self.statuses else self.status
        L, n, F = a["L"], a["N"], a["F"]
        rec = {k: a[k] for k in ("L", "N", "F", "eps", "flags")}
        rec["x"] = f32_at(a["x"], L * n * F)
        for key in ("weight", "bias", "rm", "rv"):
            rec[key] = f32_at(a[key], F)
        rec["slope"] = f32_at(a["slope"], F if a["flags"] & nm.SLOPE_PER_CHANNEL else 1)
        back = name.endswith("backward")
        if back:
            rec["gy"] = f32_at(a["gy"], L * n * F)
            rec["stat"] = None if a["stat"] is None else f64_at(a["stat"], L * 3 * F)
            rec["outs"] = tuple(a[k] is not None for k in ("gx", "gweight", "gbias", "gslope"))
        else:
            rec["momentum"] = a["momentum"]
            rec["has_stat"] = a["stat"] is not None
        self.calls.append((name, rec))
        if status:
            return status
        if back:
            fill(a["gx"], L * n * F, 3.0)
            fill(a["gweight"], F, 4.0)
            fill(a["gbias"], F, 5.0)
            fill(a["gslope"], F if a["flags"] & nm.SLOPE_PER_CHANNEL else 1, 6.0)
        else:
            fill(a["y"], L * n * F, 2.0)
            fill(a["stat"], L * 3 * F, 0.5, ctypes.c_double)
            if not a["flags"] & nm.EVAL:
                for key in ("rm", "rv"):
                    if a[key] is not None:
                        out = ctypes.cast(a[key], ctypes.POINTER(ctypes.c_float))
                        for i in range(F):
                            out[i] += 1.0
        info = a["info"]._obj
        info.rows, info.features, info.layers, info.chunks, info.arena_bytes, info.vec, info.launches = n, F, L, 1, ARENA, 1, 3
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, NormStub())


def feats(*shape):
    return torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(*shape) / 4.0 - 1.0


def test_arguments_of_the_forward_export(lib):
    x, w, b = feats(2, 5, 3), feats(3) + 2, feats(3) - 1
    rm, rv = torch.zeros(3), torch.ones(3)
    y, mean, var = ops.batch_norm(x, w, b, rm, rv, momentum=0.25, eps=1e-3, pre="relu", post="relu", return_stats=True)
    (name, c), = lib.exports()
    assert name == "rlap_batch_norm" and (c["L"], c["N"], c["F"], c["momentum"], c["eps"]) == (2, 5, 3, 0.25, 1e-3)
    assert c["flags"] == _lib.NORM_PRE_RELU | _lib.NORM_POST_RELU and c["has_stat"]
    assert c["x"] == x.reshape(-1).tolist() and c["weight"] == w.tolist() and c["bias"] == b.tolist() and c["slope"] is None
    assert c["rm"] == [0.0] * 3 and c["rv"] == [1.0] * 3
    assert y.shape == x.shape and y.dtype == torch.float32 and bool((y == 2).all()) and not y.requires_grad
    assert rm.tolist() == [1.0] * 3 and rv.tolist() == [2.0] * 3                    # updated in place
    assert mean.shape == (2, 3) and mean.dtype == torch.float64 and bool((mean == 1.0).all())      # c + m
    assert bool(((var - (4.0 - 1e-3)).abs() < 1e-12).all())                         # 1 / rstd^2 - eps
    assert ops.last_stats == {"rows": 5, "features": 3, "layers": 2, "chunks": 1, "arena_bytes": ARENA, "vec": 1, "launches": 3, "host_syncs": 0}


def test_defaults_and_a_single_view(lib):
    x = feats(5, 3)
    y = ops.batch_norm(x)
    (_, c), = lib.exports()
    assert (c["L"], c["N"], c["F"], c["momentum"], c["eps"], c["flags"]) == (1, 5, 3, 0.1, 1e-5, 0) and y.shape == (5, 3)
    assert c["weight"] is None and c["bias"] is None and c["rm"] is None and c["rv"] is None and c["slope"] is None


def test_evaluation_mode_reads_the_buffers_and_writes_none(lib):
    rm, rv = feats(3), feats(3) + 3
    y, mean, var = ops.batch_norm(feats(1, 3), running_mean=rm, running_var=rv, training=False, return_stats=True)
    (_, c), = lib.exports()
    assert c["flags"] == _lib.NORM_EVAL and not c["has_stat"] and c["rm"] == rm.tolist() and c["rv"] == rv.tolist()
    assert rm.tolist() == feats(3).tolist() and mean.tolist() == [rm.tolist()] and var.tolist() == [rv.tolist()]


@pytest.mark.parametrize("per_channel", [False, True])
def test_slope_forms(lib, per_channel):
    slope = torch.full((3,), 0.25) if per_channel else torch.tensor(0.25)
    ops.batch_norm(feats(4, 3), post="prelu", slope=slope)
    (_, c), = lib.exports()
    assert c["flags"] == _lib.NORM_POST_PRELU | (_lib.NORM_SLOPE_PER_CHANNEL if per_channel else 0)
    assert c["slope"] == [0.25] * (3 if per_channel else 1)


def test_strided_inputs_and_buffers_are_packed_and_copied_back(lib):
    x = feats(3, 5).t()
    rm = torch.zeros(6)[::2]
    ops.batch_norm(x, running_mean=rm, running_var=torch.ones(3))
    (_, c), = lib.exports()
    assert c["x"] == x.contiguous().reshape(-1).tolist() and (c["N"], c["F"]) == (5, 3) and rm.tolist() == [1.0] * 3


X = torch.zeros(5, 3)
BAD = [
    {"x": torch.zeros(5)}, {"x": torch.zeros(1, 1, 5, 3)}, {"x": torch.zeros(5, 3, dtype=torch.float64)}, {"x": [[1.0, 2.0], [3.0, 4.0]]},
    {"x": torch.zeros(1, 3)}, {"x": torch.zeros(0, 5, 3)}, {"x": torch.zeros(5, 0)}, {"x": torch.zeros(2, 4097)},      # N < 2, L, F out of range
    {"x": torch.zeros(0, 3), "training": False, "running_mean": torch.zeros(3), "running_var": torch.ones(3)},
    {"weight": torch.zeros(4)}, {"bias": torch.zeros(3, dtype=torch.float64)}, {"running_mean": torch.zeros(3, 1)}, {"running_var": [1.0] * 3},
    {"weight": torch.zeros(3, device="meta")},
    {"training": False}, {"training": False, "running_mean": torch.zeros(3)}, {"training": 1},                        # evaluation without buffers
    {"momentum": None}, {"momentum": -0.1}, {"momentum": 1.5}, {"momentum": float("nan")}, {"momentum": "0.1"}, {"momentum": True},
    {"eps": 0.0}, {"eps": -1e-5}, {"eps": float("inf")}, {"eps": float("nan")}, {"eps": None},
    {"pre": "prelu"}, {"pre": None}, {"post": "gelu"}, {"post": ("relu", "prelu")},
    {"post": "prelu"}, {"post": "prelu", "slope": 0.25}, {"post": "prelu", "slope": torch.zeros(2)},                  # PReLU without a slope
    {"post": "prelu", "slope": torch.zeros(1, dtype=torch.float64)}, {"post": "relu", "slope": torch.zeros(1)},
]


@pytest.mark.parametrize("kw", BAD)
def test_bad_arguments_raise_value_error_before_any_call(lib, monkeypatch, kw):
    def reached(*args, **kwargs):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    kw = dict(kw)
    with pytest.raises(ValueError):
        ops.batch_norm(kw.pop("x", X), **kw)
    assert lib.exports() == []


def test_the_ends_of_the_ranges_are_inside(lib):
    ops.batch_norm(torch.zeros(2, 4096), momentum=0, eps=1e-300)
    ops.batch_norm(torch.zeros(1, 1), running_mean=torch.zeros(1), running_var=torch.ones(1), training=False, momentum=1)
    assert [(c["N"], c["F"]) for _, c in lib.exports()] == [(2, 4096), (1, 1)]


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (8, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    """RLAP_E_BAD_ARG -- what the library answers to both post flags, which the strings of ops cannot express -- is a ValueError."""
    lib.status = status
    with pytest.raises(exc, match=f"status {status}"):
        ops.batch_norm(feats(4, 2))
    api = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_norm.h")).read()
    assert "if ((flags & POST_RELU) && (flags & POST_PRELU)) return false;" in api


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.batch_norm(feats(4, 2))
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_batch_norm")
    assert names[i:i + 4] == ["rlap_batch_norm", "rlap_workspace_needed", "rlap_set_workspace", "rlap_batch_norm"]


def test_autograd_calls_the_backward_export_once(lib):
    x, w, b = feats(2, 4, 3).requires_grad_(True), (feats(3) + 2).requires_grad_(True), feats(3).requires_grad_(True)
    slope = torch.tensor([0.25]).requires_grad_(True)
    y = ops.batch_norm(x, w, b, post="prelu", slope=slope, pre="relu")
    assert y.requires_grad
    gy = feats(2, 4, 3) * 0.5
    y.backward(gy)
    (fname, f), (bname, c) = lib.exports()
    assert (fname, bname) == ("rlap_batch_norm", "rlap_batch_norm_backward")
    assert (c["L"], c["N"], c["F"], c["eps"], c["flags"]) == (2, 4, 3, 1e-5, f["flags"]) and c["flags"] == _lib.NORM_PRE_RELU | _lib.NORM_POST_PRELU
    assert c["x"] == x.detach().reshape(-1).tolist() and c["gy"] == gy.reshape(-1).tolist() and c["stat"] == [0.5] * 18
    assert c["weight"] == w.tolist() and c["slope"] == [0.25] and c["outs"] == (True, True, True, True) and c["rm"] is None
    assert x.grad.shape == x.shape and bool((x.grad == 3).all()) and bool((w.grad == 4).all()) and bool((b.grad == 5).all())
    assert slope.grad.shape == (1,) and float(slope.grad) == 6.0


def test_null_gradient_outputs_are_skipped(lib):
    x, w = feats(4, 3), (feats(3) + 2).requires_grad_(True)
    ops.batch_norm(x, w, feats(3)).sum().backward()
    assert lib.exports()[1][1]["outs"] == (False, True, False, False) and bool((w.grad == 4).all())


def test_evaluation_mode_backward_reads_the_buffers(lib):
    x = feats(4, 3).requires_grad_(True)
    rm, rv = feats(3), feats(3) + 3
    ops.batch_norm(x, running_mean=rm, running_var=rv, training=False).sum().backward()
    c = lib.exports()[1][1]
    assert c["flags"] == _lib.NORM_EVAL and c["rm"] == rm.tolist() and c["rv"] == rv.tolist() and c["stat"] is None


def test_no_graph_is_recorded_without_requires_grad(lib):
    assert not ops.batch_norm(feats(4, 3)).requires_grad
    x = feats(4, 3).requires_grad_(True)
    with torch.no_grad():
        assert not ops.batch_norm(x).requires_grad
    assert [c[0] for c in lib.exports()] == ["rlap_batch_norm"] * 2


def test_norm_info_layout(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_norm_info", "NormInfo")
    assert {"rlap_batch_norm", "rlap_batch_norm_backward"} <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    flags = dict(kv.split(" = ") for kv in hdr[hdr.index("enum { RLAP_NORM_PRE_RELU") + 7:hdr.index(" };", hdr.index("enum { RLAP_NORM_PRE_RELU"))].split(", "))
    assert {k: int(v) for k, v in flags.items()} == {"RLAP_NORM_PRE_RELU": nm.PRE_RELU, "RLAP_NORM_POST_RELU": nm.POST_RELU,
                                                      "RLAP_NORM_POST_PRELU": nm.POST_PRELU, "RLAP_NORM_SLOPE_PER_CHANNEL": nm.SLOPE_PER_CHANNEL,
                                                      "RLAP_NORM_EVAL": nm.EVAL}
    assert (_lib.NORM_PRE_RELU, _lib.NORM_POST_RELU, _lib.NORM_POST_PRELU, _lib.NORM_SLOPE_PER_CHANNEL, _lib.NORM_EVAL) == (1, 2, 4, 8, 16)


# ------------------------------------------------------------------------------------------------ the module
def test_the_module_carries_batchnorm1ds_state_dict(lib):
    ours = adapters.SnapshotBatchNorm(3)
    theirs = torch.nn.BatchNorm1d(3)
    assert list(ours.state_dict()) == list(theirs.state_dict()) == ["weight", "bias", "running_mean", "running_var", "num_batches_tracked"]
    with torch.no_grad():
        theirs.weight.fill_(2.0)
        theirs.running_var.fill_(3.0)
    ours.load_state_dict(theirs.state_dict())
    assert ours.weight.tolist() == [2.0] * 3 and ours.running_var.tolist() == [3.0] * 3
    assert list(adapters.SnapshotBatchNorm(3, affine=False, track_running_stats=False).state_dict()) == []
    pr = adapters.SnapshotBatchNorm(3, post="prelu", slope_init=0.1, slope_per_channel=True)
    assert list(pr.state_dict()) == ["weight", "bias", "slope", "running_mean", "running_var", "num_batches_tracked"] and [round(v, 6) for v in pr.slope.tolist()] == [0.1] * 3
    with pytest.raises(ValueError):
        adapters.SnapshotBatchNorm(3, momentum=None)


def test_the_module_honours_train_and_eval(lib):
    bn = adapters.SnapshotBatchNorm(3, pre="relu")
    y = bn(feats(2, 4, 3))
    assert y.shape == (2, 4, 3) and int(bn.num_batches_tracked) == 2 and bn.running_mean.tolist() == [1.0] * 3
    bn(feats(4, 3))
    assert int(bn.num_batches_tracked) == 3
    bn.eval()
    bn(feats(2, 4, 3))
    flags = [c["flags"] for _, c in lib.exports()]
    assert flags == [_lib.NORM_PRE_RELU, _lib.NORM_PRE_RELU, _lib.NORM_PRE_RELU | _lib.NORM_EVAL]
    assert int(bn.num_batches_tracked) == 3 and bn.running_mean.tolist() == [2.0] * 3
    free = adapters.SnapshotBatchNorm(3, track_running_stats=False).eval()
    free(feats(4, 3))
    assert lib.exports()[-1][1]["flags"] == 0 and lib.exports()[-1][1]["rm"] is None           # batch statistics in both modes
    with pytest.raises(ValueError):
        bn(feats(4, 5))
    doc = " ".join(adapters.SnapshotBatchNorm.__doc__.split())
    assert "one view per layer and view-ordered buffer updates is the reference's behaviour" in doc
