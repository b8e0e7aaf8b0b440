"""The fused bias-activation-dropout pass and the per-row layer norm (ops.bias_act_dropout, ops.layer_norm, their four exports,
DESIGN 4.28) without a GPU:

  * the rule -- the host mirror (tests/csrc/rowops_mirror.cc, every value from rlap_amd/csrc/rlap_rowops.h, contraction off)
    against float64 torch with the mirror's own mask: torch.where(keep, act(x64 + b64) * s, 0) and
    torch.nn.functional.layer_norm followed by the activation and the mask; the gradients against float64 autograd;
  * the coin restated in Python integers, its layer convention, its kept share, and that it is not rlap_edge_drop's coin;
  * the chunk rule and the row-sum order restated in numpy, bit for bit;
  * the map and the mirror's loops in a stand-alone program under -fsanitize=address,undefined;
  * the Python -> C mapping of the four exports on a stub library, every refusal, the layout of rlap_rowops_info, the modules.

Bounds.  Epilogue forward: |y - y64| <= 2^-24 |y64| -- both sides form the same float64 value and the mirror rounds it once.
Epilogue gradients: half a float32 unit in the last place of the float64 autograd result.
Layer norm, in the form of the batch norm's bounds (test_norm_cpu.py).  Forward: |y - y64| <= 2^-24 |y64| + LN_FWD_F64 s (|xh w| +
|b|), the one rounding to float32 and the float64 rounding of two differently ordered float64 evaluations.  Gradients: half a
float32 unit of the reference plus LN_GRAD_K times the sum of the magnitudes of the gradient's terms (gx: rstd |g|, rstd |mean g|,
rstd |xh| |mean g xh|; the parameter gradients: their N L summands).  Both constants are four times the largest ratio measured
with these inputs, mirror against torch float64 on the CPU, under the cap of 1e-10.  Forward: no element of any case lies outside
the float32 rounding alone, so the measured float64 term is 0 and the bound is 2^-24 |y64|.  Gradients: 2.56e-16 at (L, N, F) =
(1, 2, 2) with p = 0.2, 1.1e-16 at (1, 40, 300), none above the half unit elsewhere.
A row of one column is left to the bit-for-bit tests: its xh is exactly 0 here, while torch's float64 kernel leaves a rounding
residue of the size of eps64 |x| rstd (6e-12 for x = 1000), which no bound in terms of |xh| covers.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import rowops_mirror as rm
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LN_FWD_MEASURED = 0.0
LN_FWD_F64 = 4 * LN_FWD_MEASURED
LN_GRAD_K_MEASURED = 2.56e-16
LN_GRAD_K = 4 * LN_GRAD_K_MEASURED
assert LN_FWD_F64 <= 1e-10 and LN_GRAD_K <= 1e-10
SHAPES = [(1, 1, 1), (3, 257, 16), (2, 513, 11), (3, 100, 33), (2, 1000, 8)]
LN_SHAPES = [(1, 2, 2), (3, 257, 16), (2, 513, 11), (3, 100, 33), (1, 40, 300), (1, 5, 1100)]
ACTS = [("none", False), ("relu", False), ("prelu", False), ("prelu", True)]
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return rm.build(tmp_path_factory.mktemp("rowops"))


def half_ulp32(ref):
    return 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)


def slope_of(d, act, per_channel):
    return None if act != "prelu" else (d["slope"] if per_channel else d["slope"][:1])


# ------------------------------------------------------------------------------------------------ the epilogue's rule
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L,n,f", SHAPES)
def test_epilogue_against_torch_float64(mirror, L, n, f, p):
    d = rm.inputs(L, n, f, 100 + n)
    seed = 7 + n
    for act, per_channel in ACTS:
        for has_bias in (True, False):
            flags = rm.flags_of(act, per_channel and f > 1, True)
            slope, bias = slope_of(d, act, per_channel and f > 1), d["bias"] if has_bias else None
            keep = rm.mask(mirror, L, n, f, p, seed)
            s = mirror.rowops_scale(mirror.rowops_threshold(p, flags))
            y = rm.forward(mirror, d["x"], bias, slope, p, seed, flags)
            g = rm.backward(mirror, d["x"], d["gy"], bias, slope, p, seed, flags)
            r = rm.restatement(d["x"], keep, s, d["gy"], bias, slope, act)
            assert (np.abs(y.astype(np.float64) - r["y"]) <= 2.0 ** -24 * np.abs(r["y"])).all(), (act, per_channel, has_bias)
            assert (y[~keep] == 0).all() and not np.signbit(y[~keep]).any()
            for key in ("gx", "gbias", "gslope"):
                if r.get(key) is not None:
                    assert (np.abs(g[key].astype(np.float64) - r[key].reshape(g[key].shape)) <= half_ulp32(r[key].reshape(g[key].shape))).all(), (key, act, per_channel, has_bias)
            assert (g["gx"][~keep] == 0).all()


# ------------------------------------------------------------------------------------------------ the layer norm's rule
def ln_grad_terms(d, r, weight, slope, gy, keep, s, act, eps=1e-5):
    x, xh, v = d["x"].astype(np.float64), r["xh"], r["v"]
    f = x.shape[-1]
    w = weight.astype(np.float64) if weight is not None else np.ones(f)
    a = slope.astype(np.float64) if slope is not None else 0.0
    rstd = 1.0 / np.sqrt(x.var(-1, keepdims=True) + eps)
    dact = np.where(v > 0, 1.0, a if act == "prelu" else 0.0) if act != "none" else np.ones_like(v)
    gv = np.where(keep, gy.astype(np.float64) * s * dact, 0.0)
    g = gv * w
    t = rstd * (np.abs(g) + np.abs(g.mean(-1, keepdims=True)) + np.abs(xh) * np.abs((g * xh).mean(-1, keepdims=True)))
    return {"gx": t, "gweight": np.abs(gv * xh).sum((0, 1)), "gbias": np.abs(gv).sum((0, 1)),
            "gslope": np.where(keep & (v <= 0), np.abs(gy * s * v), 0.0).sum((0, 1))}


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("L,n,f", LN_SHAPES)
def test_layer_norm_against_torch_float64(mirror, L, n, f, p):
    d = rm.inputs(L, n, f, 300 + n)
    seed = 11 + n
    worst_f, worst_g = 0.0, 0.0
    for post, per_channel in ACTS:
        for affine in (True, False):
            pc = per_channel and f > 1
            flags = rm.flags_of(post, pc, True)
            slope = slope_of(d, post, pc)
            w, b = (d["weight"], d["bias"]) if affine else (None, None)
            keep = rm.mask(mirror, L, n, f, p, seed)
            s = mirror.rowops_scale(mirror.rowops_threshold(p, flags))
            y, _ = rm.ln_forward(mirror, d["x"], w, b, slope, 1e-5, p, seed, flags)
            g = rm.ln_backward(mirror, d["x"], d["gy"], w, b, slope, 1e-5, p, seed, flags)
            r = rm.ln_restatement(d["x"], keep, s, d["gy"], w, b, slope, 1e-5, post)
            wm = np.abs(w.astype(np.float64)) if affine else 1.0
            bm = np.abs(b.astype(np.float64)) if affine else 0.0
            size = s * (np.abs(r["xh"]) * wm + bm)
            err = np.abs(y.astype(np.float64) - r["y"])
            excess = err - 2.0 ** -24 * np.abs(r["y"])
            worst_f = max(worst_f, float((excess / np.maximum(size, 1e-300)).max()))
            assert (excess <= LN_FWD_F64 * size).all(), (post, per_channel, affine, worst_f)
            assert np.isfinite(y).all() and (y[~keep] == 0).all()
            terms = ln_grad_terms(d, r, w, slope, d["gy"], keep, s, post)
            if post == "prelu" and not pc:
                terms["gslope"] = terms["gslope"].sum(keepdims=True)
            for key in ("gx", "gweight", "gbias", "gslope"):
                if r.get(key) is None:
                    continue
                ref = r[key].reshape(g[key].shape)
                ex = np.abs(g[key].astype(np.float64) - ref) - half_ulp32(ref)
                ratio = float((ex / np.maximum(terms[key], 1e-300)).max())
                worst_g = max(worst_g, ratio)
                assert (ex <= LN_GRAD_K * terms[key]).all(), (key, post, per_channel, affine, ratio)
    print(f"L={L} n={n} F={f} p={p}: largest float64 term ratio forward {worst_f:.3g} (bound {LN_FWD_F64:.3g}), gradients {worst_g:.3g} (bound {LN_GRAD_K:.3g})")


def test_a_constant_row_gives_no_nan(mirror):
    x = np.full((1, 3, 40), 2.5, dtype=np.float32)
    y, stat = rm.ln_forward(mirror, x)
    assert (stat[..., 0] == 2.5).all() and (stat[..., 1] == 1.0 / np.sqrt(1e-5)).all() and (y == 0).all()
    g = rm.ln_backward(mirror, x, np.ones_like(x))
    assert np.isfinite(g["gx"]).all()


# ------------------------------------------------------------------------------------------------ the coin
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def coin_keeps(seed, l, i, k, f, T, salt):
    word = mix64(mix64(((seed + l) & MASK64) ^ salt) ^ mix64((i * ((f + 3) // 4) + k // 4) & MASK64))
    return ((word >> (16 * (k % 4))) & 0xFFFF) >= T


@pytest.mark.parametrize("L,n,f,p,seed", [(2, 5, 7, 0.2, 3), (1, 3, 64, 0.5, 2 ** 64 - 1), (3, 2, 1, 0.1, 12345678901234567), (1, 2, 130, 0.999, 0)])
def test_the_coin_restated_in_python_integers(mirror, L, n, f, p, seed):
    c = rm.constants(mirror)
    assert c["salt"] == int.from_bytes(b"rowopsdo", "big") and c["salt"] != int.from_bytes(b"edgedrop", "big")
    T = mirror.rowops_threshold(p, rm.TRAINING)
    assert T == min(int(round(p * 65536.0)), 65535) and mirror.rowops_scale(T) == 1.0 / (1.0 - T / 65536.0)
    keep = rm.mask(mirror, L, n, f, p, seed)
    want = np.array([[[coin_keeps(seed, l, i, k, f, T, c["salt"]) for k in range(f)] for i in range(n)] for l in range(L)])
    assert np.array_equal(keep, want)


def test_a_layer_is_the_one_layer_call_with_seed_plus_l(mirror):
    d = rm.inputs(3, 37, 10, 5)
    flags = rm.flags_of("prelu", False, True)
    y = rm.forward(mirror, d["x"], d["bias"], d["slope"][:1], 0.3, 40, flags)
    z, _ = rm.ln_forward(mirror, d["x"], d["weight"], d["bias"], d["slope"][:1], 1e-5, 0.3, 40, flags)
    keep = rm.mask(mirror, 3, 37, 10, 0.3, 40)
    for l in range(3):
        assert np.array_equal(keep[l], rm.mask(mirror, 1, 37, 10, 0.3, 40 + l)[0])
        assert rm.forward(mirror, d["x"][l:l + 1], d["bias"], d["slope"][:1], 0.3, 40 + l, flags).tobytes() == y[l:l + 1].tobytes()
        assert rm.ln_forward(mirror, d["x"][l:l + 1], d["weight"], d["bias"], d["slope"][:1], 1e-5, 0.3, 40 + l, flags)[0].tobytes() == z[l:l + 1].tobytes()
    assert not np.array_equal(keep[0], keep[1])


def test_no_dropout_gives_the_bits_of_the_call_without_it(mirror):
    d = rm.inputs(2, 50, 9, 6)
    base = rm.forward(mirror, d["x"], d["bias"], d["slope"], 0.0, 0, rm.flags_of("prelu", True, False))
    gbase = rm.backward(mirror, d["x"], d["gy"], d["bias"], d["slope"], 0.0, 0, rm.flags_of("prelu", True, False))
    lbase, _ = rm.ln_forward(mirror, d["x"], d["weight"], d["bias"], None, 1e-5, 0.0, 0, rm.flags_of("relu", False, False))
    for p, seed, training in ((0.0, 9, True), (0.4, 9, False), (1e-9, 3, True)):
        y = rm.forward(mirror, d["x"], d["bias"], d["slope"], p, seed, rm.flags_of("prelu", True, training))
        g = rm.backward(mirror, d["x"], d["gy"], d["bias"], d["slope"], p, seed, rm.flags_of("prelu", True, training))
        assert y.tobytes() == base.tobytes() and all(g[k].tobytes() == gbase[k].tobytes() for k in g)
        assert rm.ln_forward(mirror, d["x"], d["weight"], d["bias"], None, 1e-5, p, seed, rm.flags_of("relu", False, training))[0].tobytes() == lbase.tobytes()
    dropped = rm.forward(mirror, d["x"], d["bias"], d["slope"], 0.4, 9, rm.flags_of("prelu", True, True))
    assert dropped.tobytes() != base.tobytes()


@pytest.mark.parametrize("p", [0.1, 0.2, 0.5])
def test_kept_share_over_2_20_elements(mirror, p):
    """The seed is fixed and the bound is binomial, so this is deterministic."""
    n = 1 << 20
    keep = rm.mask(mirror, 2, n // 128, 64, p, 2024)
    q = 1.0 - mirror.rowops_threshold(p, rm.TRAINING) / 65536.0
    assert abs(keep.mean() - q) <= 4.0 * np.sqrt(q * (1.0 - q) / n)


def test_the_coin_is_not_the_edge_drop_coin(mirror):
    """Under the same seed the row pass keeps element e and rlap_edge_drop (view 0, uniform, the same p) keeps row e independently:
    over 2^17 places the two decisions agree at the rate of independent coins, q^2 + (1 - q)^2, within four standard deviations."""
    n, seed, p = 1 << 17, 99, 0.5
    T = mirror.rowops_threshold(p, rm.TRAINING)
    q = 1.0 - T / 65536.0
    ours = rm.mask(mirror, 1, n // 64, 64, p, seed).reshape(-1)
    view = mix64(seed ^ int.from_bytes(b"edgedrop", "big"))
    theirs = np.array([(mix64(view ^ mix64(e)) >> 11) * 2.0 ** -53 >= p for e in range(n)])
    agree = q * q + (1.0 - q) * (1.0 - q)
    assert abs((ours == theirs).mean() - agree) <= 4.0 * np.sqrt(agree * (1.0 - agree) / n)
    src = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_edgedrop.h")).read()
    assert "COIN_SALT = 0x6564676564726F70ull" in src and "mix64((seed + (uint64_t)k) ^ COIN_SALT)" in src


# ------------------------------------------------------------------------------------------------ the orders, restated
def chunk_rule(terms):
    total = np.float64(0.0)
    for b in range(0, len(terms), 256):
        c = np.float64(0.0)
        for t in terms[b:b + 256]:
            c = c + t
        total = total + c
    return total


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_the_chunk_rule_restated_in_numpy(mirror, n):
    d = rm.inputs(2, n, 6, n)
    flags = rm.flags_of("prelu", True, True)
    keep = rm.mask(mirror, 2, n, 6, 0.25, 5)
    s = np.float64(mirror.rowops_scale(mirror.rowops_threshold(0.25, flags)))
    g = rm.backward(mirror, d["x"], d["gy"], d["bias"], d["slope"], 0.25, 5, flags)
    x, gy = d["x"].astype(np.float64), d["gy"].astype(np.float64)
    for k in range(6):
        a = np.float64(d["slope"][k])
        A, C = np.float64(0.0), np.float64(0.0)
        for l in range(2):
            v = x[l, :, k] + np.float64(d["bias"][k])
            t = gy[l, :, k] * s
            A = A + chunk_rule(np.where(keep[l, :, k], t * np.where(v > 0, 1.0, a), 0.0))
            C = C + chunk_rule(np.where(keep[l, :, k] & (v <= 0), t * v, 0.0))
        assert np.float32(A).tobytes() == g["gbias"][k].tobytes() and np.float32(C).tobytes() == g["gslope"][k].tobytes(), k


def row_sum(terms):
    f = len(terms)
    part = np.zeros(64)
    for t in range(64):
        acc = np.float64(0.0)
        for m in range((f + 255) // 256):
            for v in range(4):
                k = 256 * m + 4 * t + v
                if k < f:
                    acc = acc + terms[k]
        part[t] = acc
    off = 32
    while off:
        part = part + part[np.arange(64) ^ off]
        off >>= 1
    return part[0]


@pytest.mark.parametrize("f", [1, 3, 4, 63, 64, 65, 100, 256, 257, 1024, 4096])
def test_the_row_sum_order_restated_in_numpy(mirror, f):
    terms = np.random.RandomState(f).standard_normal(f) * 10.0 ** np.random.RandomState(f + 1).randint(-3, 4, f)
    want = row_sum(terms)
    assert np.float64(rm.row_sum(mirror, terms)).tobytes() == np.float64(want).tobytes()
    x = terms.astype(np.float32)[None, None, :]
    _, stat = rm.ln_forward(mirror, x)
    mean = row_sum(x[0, 0].astype(np.float64)) / np.float64(f)
    d = x[0, 0].astype(np.float64) - mean
    rstd = np.float64(1.0) / np.sqrt(row_sum(d * d) / np.float64(f) + np.float64(1e-5))
    assert np.array([mean, rstd]).tobytes() == stat[0, 0].tobytes()
    assert mirror.rowops_ln_lg(f) == min(6, max(0, int(np.ceil(np.log2(max(1, (f + 3) // 4))))))
    assert mirror.rowops_ln_instance(f) == 1 << max(0, int(np.ceil(np.log2((f + 255) // 256))))


# ------------------------------------------------------------------------------------------------ the map, under the sanitizers
def test_the_map_functions_and_the_loops_under_asan_ubsan(tmp_path):
    exe = tmp_path / "rowops_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "rowops_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "600"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " sizes, 0 failures" in r.stdout


def test_constants_and_arena_sizes(mirror):
    c = rm.constants(mirror)
    assert c["chunk"] == 256 and c["max_f"] == _lib.ROW_MAX_F == ops.ROW_MAX_F == 4096
    src = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_rowops.hip")).read()
    assert "RO_MAX_GRID = norm::MAX_GRID" in src and "RO_WAVES = norm::GROUP_WAVES" in src     # the launchers read the header's
    piece = lambda doubles: (doubles * 8 + 255) // 256 * 256
    assert mirror.rowops_backward_bytes(3, 513, 33, 0, 0) == 0
    assert mirror.rowops_backward_bytes(3, 513, 33, 1, 0) == piece(3 * 3 * 33) + piece(3 * 33)
    assert mirror.rowops_backward_bytes(3, 513, 33, 0, 1) == piece(2 * 3 * 3 * 33) + piece(2 * 3 * 33)
    assert mirror.rowops_ln_backward_bytes(3, 513, 33, 0, 0, 0) == 0
    assert mirror.rowops_ln_backward_bytes(3, 513, 33, 1, 0, 0) == piece(2 * 3 * 3 * 33) + piece(2 * 3 * 33) + piece(2 * 3 * 513)
    assert mirror.rowops_ln_backward_bytes(3, 513, 33, 0, 0, 1) == piece(3 * 3 * 3 * 33) + piece(3 * 3 * 33) + piece(2 * 3 * 513)
    assert mirror.rowops_split_of(10, 1) == 0 and mirror.rowops_split_of(10, 0) == 4 and mirror.rowops_split_of(5000, 0) == 0


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_bias_act_dropout": "h x L N F bias slope p seed flags y info",
    "rlap_bias_act_dropout_backward": "h x gy L N F bias slope p seed flags gx gbias gslope info",
    "rlap_layer_norm": "h x L N F weight bias slope eps p seed flags y info",
    "rlap_layer_norm_backward": "h x gy L N F weight bias slope eps p seed flags gx gweight gbias gslope info",
}
ARENA = 4321


def f32_at(addr, count):
    return None if addr is None else list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


def fill(addr, count, value):
    if addr is not None:
        out = ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))
        for i in range(count):
            out[i] = value


class RowStub(StubLib):
    """Records the four exports; a forward writes y = 2; a backward gx = 3, gweight = 4, gbias = 5, gslope = 6."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        status = self.statuses.pop(0) if self.statuses else self.status
        L, n, F = a["L"], a["N"], a["F"]
        rec = {k: a[k] for k in ("L", "N", "F", "p", "seed", "flags")}
        rec["eps"] = a.get("eps")
        rec["x"] = f32_at(a["x"], L * n * F)
        rec["bias"] = f32_at(a["bias"], F)
        rec["weight"] = f32_at(a.get("weight"), F)
        rec["slope"] = f32_at(a["slope"], F if a["flags"] & rm.SLOPE_PER_CHANNEL else 1)
        back = name.endswith("backward")
        slots = F if a["flags"] & rm.SLOPE_PER_CHANNEL else 1
        if back:
            rec["gy"] = f32_at(a["gy"], L * n * F)
            rec["outs"] = tuple(a.get(k) is not None for k in ("gx", "gweight", "gbias", "gslope"))
        self.calls.append((name, rec))
        if status:
            return status
        if back:
            fill(a["gx"], L * n * F, 3.0)
            fill(a.get("gweight"), F, 4.0)
            fill(a["gbias"], F, 5.0)
            fill(a["gslope"], slots, 6.0)
        else:
            fill(a["y"], L * n * F, 2.0)
        info = a["info"]._obj
        info.rows, info.features, info.layers, info.chunks, info.arena_bytes, info.vec, info.launches, info.instance = n, F, L, 1, ARENA, 1, 3, 2
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, RowStub())


def feats(*shape):
    return torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(*shape) / 4.0 - 1.0


def test_arguments_of_the_epilogue_forward(lib):
    x, b = feats(2, 5, 3), feats(3) - 1
    y = ops.bias_act_dropout(x, b, act="relu", p=0.25, seed=-1)
    (name, c), = lib.exports()
    assert name == "rlap_bias_act_dropout" and (c["L"], c["N"], c["F"], c["p"], c["seed"]) == (2, 5, 3, 0.25, 2 ** 64 - 1)
    assert c["flags"] == _lib.ROW_ACT_RELU | _lib.ROW_TRAINING and c["x"] == x.reshape(-1).tolist() and c["bias"] == b.tolist() and c["slope"] is None
    assert y.shape == x.shape and y.dtype == torch.float32 and bool((y == 2).all()) and not y.requires_grad
    assert ops.last_stats == {"rows": 5, "features": 3, "layers": 2, "chunks": 1, "arena_bytes": ARENA, "vec": 1, "launches": 3, "instance": 2, "host_syncs": 0}


def test_defaults_and_a_single_view(lib):
    y = ops.bias_act_dropout(feats(5, 3))
    z = ops.layer_norm(feats(5, 3))
    (_, c), (_, e) = lib.exports()
    assert (c["L"], c["N"], c["F"], c["p"], c["seed"], c["flags"]) == (1, 5, 3, 0.0, 0, _lib.ROW_TRAINING) and y.shape == (5, 3)
    assert (e["L"], e["N"], e["F"], e["p"], e["seed"], e["flags"], e["eps"]) == (1, 5, 3, 0.0, 0, _lib.ROW_TRAINING, 1e-5) and z.shape == (5, 3)
    assert c["bias"] is None and c["slope"] is None and e["weight"] is None and e["bias"] is None


def test_arguments_of_the_layer_norm_forward(lib):
    x, w, b = feats(2, 5, 3), feats(3) + 2, feats(3) - 1
    ops.layer_norm(x, w, b, eps=1e-3, post="prelu", slope=torch.full((3,), 0.25), p=0.5, training=False, seed=9)
    (name, c), = lib.exports()
    assert name == "rlap_layer_norm" and (c["eps"], c["p"], c["seed"]) == (1e-3, 0.5, 9)
    assert c["flags"] == _lib.ROW_ACT_PRELU | _lib.ROW_SLOPE_PER_CHANNEL and c["weight"] == w.tolist() and c["bias"] == b.tolist() and c["slope"] == [0.25] * 3


def test_seed_none_draws_from_torchs_generator_only_when_it_drops(lib):
    torch.manual_seed(5)
    ops.bias_act_dropout(feats(4, 3), p=0.5, seed=None)
    ops.bias_act_dropout(feats(4, 3), p=0.5, seed=None)
    torch.manual_seed(5)
    ops.bias_act_dropout(feats(4, 3), p=0.5, seed=None)
    state = torch.get_rng_state()
    ops.bias_act_dropout(feats(4, 3), p=0.0, seed=None)
    ops.bias_act_dropout(feats(4, 3), p=0.5, seed=None, training=False)
    assert torch.equal(state, torch.get_rng_state())
    seeds = [c["seed"] for _, c in lib.exports()]
    assert seeds[0] != seeds[1] and seeds[2] == seeds[0] and seeds[3:] == [0, 0]


X = torch.zeros(5, 3)
BAD = [
    {"x": torch.zeros(5)}, {"x": torch.zeros(1, 1, 5, 3)}, {"x": torch.zeros(5, 3, dtype=torch.float64)}, {"x": [[1.0, 2.0], [3.0, 4.0]]},
    {"x": torch.zeros(0, 5, 3)}, {"x": torch.zeros(0, 3)}, {"x": torch.zeros(5, 0)}, {"x": torch.zeros(2, 4097)},
    {"bias": torch.zeros(4)}, {"bias": torch.zeros(3, dtype=torch.float64)}, {"bias": [0.0] * 3}, {"bias": torch.zeros(3, device="meta")},
    {"training": 1}, {"p": -0.1}, {"p": 1.0}, {"p": 1.5}, {"p": float("nan")}, {"p": "0.1"}, {"p": True}, {"p": None},
    {"seed": 1.5}, {"seed": "7"}, {"seed": True},
]
BAD_ACT = [{"A": "gelu"}, {"A": None}, {"A": ("relu", "prelu")}, {"A": "prelu"}, {"A": "prelu", "slope": 0.25}, {"A": "prelu", "slope": torch.zeros(2)},
           {"A": "prelu", "slope": torch.zeros(1, dtype=torch.float64)}, {"A": "relu", "slope": torch.zeros(1)}]


def unreachable(monkeypatch):
    def reached(*args, **kwargs):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)


@pytest.mark.parametrize("kw", BAD + BAD_ACT)
def test_bad_epilogue_arguments_raise_value_error_before_any_call(lib, monkeypatch, kw):
    unreachable(monkeypatch)
    kw = {("act" if k == "A" else k): v for k, v in kw.items()}
    with pytest.raises(ValueError):
        ops.bias_act_dropout(kw.pop("x", X), **kw)
    assert lib.exports() == []


@pytest.mark.parametrize("kw", BAD + BAD_ACT + [{"weight": torch.zeros(4)}, {"weight": [1.0] * 3}, {"eps": 0.0}, {"eps": -1e-5}, {"eps": float("inf")},
                                                {"eps": float("nan")}, {"eps": None}, {"eps": True}])
def test_bad_layer_norm_arguments_raise_value_error_before_any_call(lib, monkeypatch, kw):
    unreachable(monkeypatch)
    kw = {("post" if k == "A" else k): v for k, v in kw.items()}
    with pytest.raises(ValueError):
        ops.layer_norm(kw.pop("x", X), **kw)
    assert lib.exports() == []


def test_the_ends_of_the_ranges_are_inside(lib):
    ops.bias_act_dropout(torch.zeros(1, 4096), p=0.999999)
    ops.layer_norm(torch.zeros(1, 1), eps=1e-300)
    assert [(c["N"], c["F"]) for _, c in lib.exports()] == [(1, 4096), (1, 1)]


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (8, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    with pytest.raises(exc, match=f"status {status}"):
        ops.bias_act_dropout(feats(4, 2))
    with pytest.raises(exc, match=f"status {status}"):
        ops.layer_norm(feats(4, 2))
    api = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_rowops.h")).read()
    assert "if ((flags & ACT_RELU) && (flags & ACT_PRELU)) return false;" in api


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.layer_norm(feats(4, 2))
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_layer_norm")
    assert names[i:i + 4] == ["rlap_layer_norm", "rlap_workspace_needed", "rlap_set_workspace", "rlap_layer_norm"]


def test_autograd_calls_the_epilogue_backward_once_with_the_saved_seed(lib):
    x, b = feats(2, 4, 3).requires_grad_(True), feats(3).requires_grad_(True)
    slope = torch.tensor([0.25]).requires_grad_(True)
    torch.manual_seed(3)
    y = ops.bias_act_dropout(x, b, act="prelu", slope=slope, p=0.5, seed=None)
    assert y.requires_grad
    gy = feats(2, 4, 3) * 0.5
    y.backward(gy)
    (fname, f), (bname, c) = lib.exports()
    assert (fname, bname) == ("rlap_bias_act_dropout", "rlap_bias_act_dropout_backward")
    assert (c["L"], c["N"], c["F"], c["p"], c["seed"], c["flags"]) == (2, 4, 3, 0.5, f["seed"], f["flags"]) and f["seed"] != 0
    assert c["x"] == x.detach().reshape(-1).tolist() and c["gy"] == gy.reshape(-1).tolist() and c["bias"] == b.tolist() and c["slope"] == [0.25]
    assert c["outs"] == (True, False, True, True)
    assert x.grad.shape == x.shape and bool((x.grad == 3).all()) and bool((b.grad == 5).all()) and slope.grad.shape == (1,) and float(slope.grad) == 6.0


def test_autograd_calls_the_layer_norm_backward_once(lib):
    x, w, b = feats(2, 4, 3).requires_grad_(True), (feats(3) + 2).requires_grad_(True), feats(3).requires_grad_(True)
    slope = torch.full((3,), 0.25).requires_grad_(True)
    ops.layer_norm(x, w, b, eps=1e-4, post="prelu", slope=slope, p=0.25, seed=77).backward(feats(2, 4, 3))
    (_, f), (bname, c) = lib.exports()
    assert bname == "rlap_layer_norm_backward" and (c["eps"], c["p"], c["seed"], c["flags"]) == (1e-4, 0.25, 77, f["flags"])
    assert c["weight"] == w.tolist() and c["outs"] == (True, True, True, True)
    assert bool((x.grad == 3).all()) and bool((w.grad == 4).all()) and bool((b.grad == 5).all()) and slope.grad.tolist() == [6.0] * 3


def test_null_gradient_outputs_are_skipped(lib):
    b = feats(3).requires_grad_(True)
    ops.bias_act_dropout(feats(4, 3), b).sum().backward()
    w = (feats(3) + 2).requires_grad_(True)
    ops.layer_norm(feats(4, 3), w, feats(3)).sum().backward()
    x = feats(4, 3).requires_grad_(True)
    ops.layer_norm(x, feats(3), feats(3)).sum().backward()
    outs = [c["outs"] for name, c in lib.exports() if name.endswith("backward")]
    assert outs == [(False, False, True, False), (False, True, False, False), (True, False, False, False)]


def test_no_graph_is_recorded_without_requires_grad(lib):
    assert not ops.bias_act_dropout(feats(4, 3)).requires_grad
    x = feats(4, 3).requires_grad_(True)
    with torch.no_grad():
        assert not ops.layer_norm(x).requires_grad
    assert [c[0] for c in lib.exports()] == ["rlap_bias_act_dropout", "rlap_layer_norm"]


def test_rowops_info_layout(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_rowops_info", "RowopsInfo")
    assert set(SIGS) <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    at = hdr.index("enum { RLAP_ROW_ACT_RELU")
    flags = dict(kv.split(" = ") for kv in hdr[at + 7:hdr.index(" };", at)].split(", "))
    assert {k: int(v) for k, v in flags.items()} == {"RLAP_ROW_ACT_RELU": rm.ACT_RELU, "RLAP_ROW_ACT_PRELU": rm.ACT_PRELU,
                                                      "RLAP_ROW_SLOPE_PER_CHANNEL": rm.SLOPE_PER_CHANNEL, "RLAP_ROW_TRAINING": rm.TRAINING}
    assert (_lib.ROW_ACT_RELU, _lib.ROW_ACT_PRELU, _lib.ROW_SLOPE_PER_CHANNEL, _lib.ROW_TRAINING) == (1, 2, 4, 8)


# ------------------------------------------------------------------------------------------------ the modules
def test_state_dicts_of_the_modules(lib):
    act, theirs = adapters.SnapshotActDropout("prelu", 0.2, num_parameters=3), torch.nn.PReLU(3)
    assert list(act.state_dict()) == list(theirs.state_dict()) == ["weight"] and act.weight.tolist() == [0.25] * 3
    with torch.no_grad():
        theirs.weight.fill_(0.5)
    act.load_state_dict(theirs.state_dict())
    assert act.weight.tolist() == [0.5] * 3 and list(adapters.SnapshotActDropout("relu", 0.1).state_dict()) == []
    ln, theirs = adapters.SnapshotLayerNorm(3), torch.nn.LayerNorm(3)
    assert list(ln.state_dict()) == list(theirs.state_dict()) == ["weight", "bias"]
    with torch.no_grad():
        theirs.weight.fill_(2.0)
    ln.load_state_dict(theirs.state_dict())
    assert ln.weight.tolist() == [2.0] * 3 and list(adapters.SnapshotLayerNorm(3, elementwise_affine=False).state_dict()) == []
    assert list(adapters.SnapshotLayerNorm(3, post="prelu", p=0.2).state_dict()) == ["weight", "bias", "slope"]
    enc = adapters.SnapshotG2LEncoder(5, 8, 2, encoder_norm="layer", projector_norm="batch")
    names = list(enc.state_dict())
    assert "activation.weight" in names and "batch_norm.weight" in names and "head_norm.slope" in names and "head_norm.running_mean" in names
    for bad in ({"act": "gelu"}, {"p": 1.0}, {"p": -0.5}):
        with pytest.raises(ValueError):
            adapters.SnapshotActDropout(**bad)
    with pytest.raises(ValueError):
        adapters.SnapshotG2LEncoder(5, 8, 2, encoder_norm="group")


def test_eval_switches_the_dropout_off(lib):
    act, ln = adapters.SnapshotActDropout("prelu", 0.2, seed=4), adapters.SnapshotLayerNorm(3, post="relu", p=0.3, seed=5)
    act(feats(2, 4, 3), feats(3))
    ln(feats(4, 3))
    act.eval()
    ln.eval()
    act(feats(2, 4, 3))
    ln(feats(4, 3))
    calls = [c for _, c in lib.exports()]
    assert [c["flags"] for c in calls] == [_lib.ROW_ACT_PRELU | _lib.ROW_TRAINING, _lib.ROW_ACT_RELU | _lib.ROW_TRAINING, _lib.ROW_ACT_PRELU, _lib.ROW_ACT_RELU]
    assert [c["seed"] for c in calls] == [4, 5, 4, 5] and [c["p"] for c in calls] == [0.2, 0.3, 0.2, 0.3]
    assert calls[0]["bias"] == feats(3).tolist() and calls[2]["bias"] is None and calls[0]["slope"] == [0.25]
    with pytest.raises(ValueError):
        ln(feats(4, 5))


def test_a_module_without_a_seed_draws_a_fresh_one_every_training_forward(lib):
    act = adapters.SnapshotActDropout("none", 0.5)
    act(feats(4, 3))
    act(feats(4, 3))
    a, b = (c["seed"] for _, c in lib.exports())
    assert a != b


class Holder:
    """A snapshot holder by duck typing: two layers, the identity as propagation."""

    def propagate(self, x, transpose=False):
        return torch.stack([x, x]) if x.dim() == 2 else x


def test_gcn_conv_without_an_epilogue_is_what_it_was(lib):
    conv = adapters.SnapshotGCNConv(3, 2)
    with torch.no_grad():
        conv.bias.copy_(torch.tensor([0.5, -0.5]))
    x = feats(4, 3)
    y = conv(x, Holder())
    assert lib.exports() == [] and conv.epilogue is None and list(conv.state_dict()) == ["weight", "bias"]
    assert torch.equal(y, torch.stack([x @ conv.weight, x @ conv.weight]) + conv.bias)
    fused = adapters.SnapshotGCNConv(3, 2, epilogue=adapters.SnapshotActDropout("prelu", 0.1, seed=3))
    fused.load_state_dict(conv.state_dict(), strict=False)
    fused(x, Holder())
    (name, c), = lib.exports()
    assert name == "rlap_bias_act_dropout" and (c["L"], c["N"], c["F"]) == (2, 4, 2) and c["bias"] == [0.5, -0.5] and c["seed"] == 3
    assert c["x"] == torch.stack([x @ conv.weight, x @ conv.weight]).reshape(-1).tolist()
    assert list(fused.state_dict()) == ["weight", "bias", "epilogue.weight"]
    with pytest.raises(ValueError):
        adapters.SnapshotGCNConv(3, 2, epilogue=torch.nn.PReLU())


def test_update_target_is_the_moving_average():
    a, b = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    want = [0.75 * p.data + 0.25 * q.data for p, q in zip(a.parameters(), b.parameters())]
    adapters.update_target(a, b, 0.75)
    assert all(torch.allclose(p.data, w, rtol=0, atol=1e-7) for p, w in zip(a.parameters(), want))
    with pytest.raises(ValueError):
        adapters.update_target(a, torch.nn.Linear(3, 2, bias=False), 0.5)
