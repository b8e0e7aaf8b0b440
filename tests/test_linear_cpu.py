"""The fused dense layer (ops.linear_act, rlap_linear_act / rlap_linear_act_backward) without a GPU:

  * the rule -- the host mirror (tests/csrc/linear_mirror.cc, every value from rlap_amd/csrc/rlap_linear.h, contraction off) against
    a float64 restatement in numpy, for every activation, with and without a bias; the order's invariances;
  * the work maps of the header over every (Fin, Fout) in [1, 512]^2 and a sweep of M;
  * the index arithmetic and the mirror in a stand-alone program under -fsanitize=address,undefined;
  * the Python -> C mapping of both exports on a stub library, the layout of rlap_linear_info, the adapters.

The bounds against the restatement are derived, not measured, with u = 2^-24, Fp = the inner width padded to 32:
  y, act none / relu (relu is 1-Lipschitz):  |y - y64| <= (Finp + 2) u (sum_k |x_ik W_ko| + |b_o|) -- a float32 fmaf chain of length
      Finp (gamma_n <= n u) and the two roundings;
  y, act elu:  max(1, alpha) times that (ELU's Lipschitz constant) plus u |y| for expm1 and its rounding;
  gx:  (Foutp + 2) u sum_o |t_io W_ko|, the same chain over o and the rounding of t;
  gW:  (rows of the longest part + parts + 2) u sum_i |x_ik t_io| -- the chain of a part, the float64 sum of the parts, the roundings;
  gb:  u |gb| + 1e-13 sum_i |t_io| against the float64 sum of the float32 t, as the chunk rule's other users.
The backward restatement starts from the stored float32 y and gy, as the rule does.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import linear_mirror as lm
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return lm.build(tmp_path_factory.mktemp("linear"))


def pad32(f):
    return (f + 31) // 32 * 32


def same(x, y):
    return np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()


# ------------------------------------------------------------------------------------------------ the rule
SHAPES = [(1, 1, 1), (33, 3, 5), (65, 33, 31), (129, 64, 64), (300, 100, 257), (40, 512, 512), (2049, 20, 12)]


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("act,alpha", [("none", 1.0), ("relu", 1.0), ("elu", 1.0), ("elu", 2.5)])
@pytest.mark.parametrize("m,fin,fout", SHAPES)
def test_mirror_against_the_float64_restatement(mirror, m, fin, fout, act, alpha, bias):
    x, w, b, gy = lm.inputs(m, fin, fout, 100 + m + fin, bias)
    y = lm.forward(mirror, x, w, b, act, alpha)
    y64, v64, a = lm.restatement(x, w, b, act, alpha)
    bound = (pad32(fin) + 2) * U * a
    if act == "elu":
        bound = max(1.0, alpha) * bound + U * np.abs(y64)
    err = np.abs(y.astype(np.float64) - y64)
    print(f"m={m} {fin}->{fout} {act}: forward worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all()
    if act != "none" and m * fout >= 100:
        assert (v64 > 0).any() and (v64 < 0).any()                       # both branches are met

    g = lm.backward(mirror, x, w, y, gy, act, alpha)
    gx64, gw64, _, ax, aw, t64 = lm.restatement_backward(x, w, y, gy, act, alpha)
    parts = mirror.lin_num_parts(m, fin, fout)
    longest = max(mirror.lin_part_begin(m, fin, fout, p + 1) - mirror.lin_part_begin(m, fin, fout, p) for p in range(parts))
    ex = np.abs(g["gx"].astype(np.float64) - gx64)
    ew = np.abs(g["gw"].astype(np.float64) - gw64)
    t32 = t64.astype(np.float32).astype(np.float64)
    eb = np.abs(g["gb"].astype(np.float64) - t32.sum(0))
    bx, bw, bb = (pad32(fout) + 2) * U * ax, (longest + parts + 2) * U * aw, U * np.abs(t32.sum(0)) + 1e-13 * np.abs(t32).sum(0)
    print(f"    gx {np.max(ex / np.maximum(bx, 1e-300)):.3g}, gW {np.max(ew / np.maximum(bw, 1e-300)):.3g}, "
          f"gb {np.max(eb / np.maximum(bb, 1e-300)):.3g} of their bounds ({parts} parts, longest {longest} rows)")
    assert (ex <= bx).all() and (ew <= bw).all() and (eb <= bb).all()


# ------------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("act", ["none", "relu", "elu"])
def test_a_layered_call_is_the_call_on_its_rows(mirror, act):
    x, w, b, gy = lm.inputs(3 * 45, 33, 20, 5)
    y2 = lm.forward(mirror, x, w, b, act)
    y3 = lm.forward(mirror, x.reshape(3, 45, 33), w, b, act)
    assert y3.shape == (3, 45, 20) and same(y2, y3)
    g2 = lm.backward(mirror, x, w, y2, gy, act)
    g3 = lm.backward(mirror, x.reshape(3, 45, 33), w, y3, gy.reshape(3, 45, 20), act)
    assert all(same(g2[k], g3[k]) for k in ("gx", "gw", "gb"))


@pytest.mark.parametrize("act", ["none", "relu", "elu"])
@pytest.mark.parametrize("m,fin,fout", [(33, 3, 5), (65, 33, 64), (129, 100, 31)])
def test_weight_out_in_on_the_transpose_is_the_plain_call(mirror, m, fin, fout, act):
    x, w, b, gy = lm.inputs(m, fin, fout, 9)
    wt = np.ascontiguousarray(w.T)
    y = lm.forward(mirror, x, w, b, act, 0.75)
    assert same(y, lm.forward(mirror, x, wt, b, act, 0.75, out_in=True))
    g, gt = lm.backward(mirror, x, w, y, gy, act, 0.75), lm.backward(mirror, x, wt, y, gy, act, 0.75, out_in=True)
    assert same(g["gx"], gt["gx"]) and same(g["gb"], gt["gb"]) and same(g["gw"], gt["gw"].T) and gt["gw"].shape == (fout, fin)


@pytest.mark.parametrize("bias", [True, False])
def test_relu_is_none_followed_by_the_clamp(mirror, bias):
    x, w, b, _ = lm.inputs(129, 33, 65, 13, bias)
    y0 = lm.forward(mirror, x, w, b, "none")
    assert same(lm.forward(mirror, x, w, b, "relu"), np.where(y0 > 0, y0, np.float32(0.0)))
    assert (y0 < 0).any()


def test_threads_and_zero_columns_change_no_bit(mirror):
    x, w, b, gy = lm.inputs(65, 33, 31, 17)
    y = lm.forward(mirror, x, w, b, "elu")
    g = lm.backward(mirror, x, w, y, gy, "elu")
    for threads, pad in ((1, 0), (3, 1), (8, 3)):
        assert same(y, lm.forward(mirror, x, w, b, "elu", threads=threads, pad_tiles=pad))
        o = lm.backward(mirror, x, w, y, gy, "elu", threads=threads, pad_tiles=pad)
        assert all(same(g[k], o[k]) for k in ("gx", "gw", "gb"))


def test_optional_gradients_and_the_saved_values(mirror):
    """Each gradient alone equals its value in the full call; the backward reads the STORED y: under relu a y of +0 gives t = 0."""
    x, w, b, gy = lm.inputs(40, 5, 7, 3)
    y = lm.forward(mirror, x, w, b, "relu")
    g = lm.backward(mirror, x, w, y, gy, "relu")
    for key in ("gx", "gw", "gb"):
        o = lm.backward(mirror, x, w, y, gy, "relu", want=(key,))
        assert same(o[key], g[key]) and all(o[k] is None for k in o if k != key)
    dead = lm.backward(mirror, x, w, np.zeros_like(y), gy, "relu")
    assert not dead["gx"].any() and not dead["gw"].any() and not dead["gb"].any()
    alive = lm.backward(mirror, x, w, np.zeros_like(y), gy, "elu", alpha=0.5)          # d = y + alpha = 0.5
    assert same(alive["gb"], lm.backward(mirror, x, w, y, (0.5 * gy).astype(np.float32), "none")["gb"])


# ------------------------------------------------------------------------------------------------ the work maps
def test_parts_over_every_width_and_a_sweep_of_rows(mirror):
    """The parts depend on (Fin, Fout) through the tile counts alone -- asserted over all of [1, 512]^2 --, and for every pair of tile
    counts and every M of the sweep they are contiguous, multiples of 32 and cover [0, padded_rows(M))."""
    ms = [1, 31, 32, 33, 127, 128, 129, 300, 2049, 2708, 4245, 169343, 3 * 4194304, 2 ** 31 - 1]
    tiles = lambda f: (f + 31) // 32
    by_tiles = {}
    for fin in range(1, 513):
        for fout in range(1, 513):
            p = mirror.lin_num_parts(2049, fin, fout)
            assert by_tiles.setdefault((tiles(fin), tiles(fout)), p) == p
    assert len(by_tiles) == 256
    for (ti, to) in by_tiles:
        fin, fout = 32 * ti, 32 * to - 31
        groups = mirror.lin_pair_groups(fin, fout)
        assert groups == ((ti + 1) // 2) * ((((to + 1) // 2) + 3) // 4)
        for m in ms:
            p, t = mirror.lin_num_parts(m, fin, fout), (m + 31) // 32
            assert 1 <= p <= min(t, 1024) and p == max(1, min(t, 1024, -(-1024 // groups)))
            begins = [mirror.lin_part_begin(m, fin, fout, q) for q in range(p + 1)]
            assert begins[0] == 0 and begins[-1] == 32 * t and all(b % 32 == 0 for b in begins)
            assert all(lo < hi for lo, hi in zip(begins, begins[1:]))
    assert mirror.lin_num_parts(2049, 32, 32) == 65 and mirror.lin_num_parts(2112, 512, 512) == 64 and mirror.lin_num_parts(129, 64, 64) == 5
    assert mirror.lin_num_parts(3 * 4194304, 64, 64) == 1024 and mirror.lin_num_parts(3 * 4194304, 256, 256) == 256


def test_every_tile_is_owned_by_exactly_one_wave(mirror):
    assert [mirror.lin_col_waves(t) for t in range(1, 17)] == [1, 2] + [4] * 14
    assert [mirror.lin_product_instance(t) for t in range(0, 18)] == [0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 0]
    assert [mirror.lin_cross_instance(t) for t in range(0, 18)] == [0, 1, 1, 2, 2] + [4] * 12 + [0]
    for nct in range(1, 17):
        cw, rt, inst = mirror.lin_col_waves(nct), mirror.lin_row_tiles(nct), mirror.lin_product_instance(nct)
        assert cw * rt == 4
        for m in (1, 32, 33, 129, 300, 2049):
            t = (m + 31) // 32
            groups = mirror.lin_product_groups(m, nct)
            owned = {}
            for g in range(groups):
                for w in range(4):
                    row = mirror.lin_wave_row_tile(g, w, nct)
                    assert mirror.lin_wave_col_tile(w, inst, nct) >= nct          # the instance holds the wave's tiles
                    for j in range(inst):
                        col = mirror.lin_wave_col_tile(w, j, nct)
                        if col < nct and row < t:
                            owned[(row, col)] = owned.get((row, col), 0) + 1
            assert owned == {(r, c): 1 for r in range(t) for c in range(nct)}


def test_ranges(mirror):
    assert all(mirror.lin_alpha_ok(a) for a in (1e-300, 0.5, 1.0, 1e300))
    assert not any(mirror.lin_alpha_ok(a) for a in (0.0, -1.0, float("nan"), float("inf"), -float("inf")))
    assert mirror.lin_flags_ok(0) and mirror.lin_flags_ok(1) and not mirror.lin_flags_ok(2) and not mirror.lin_flags_ok(-1)
    assert [mirror.lin_act_ok(a) for a in (-1, 0, 1, 2, 3)] == [0, 1, 1, 1, 0]
    assert mirror.lin_vec_ok(64, 0x1000) and not mirror.lin_vec_ok(64, 0x1004) and not mirror.lin_vec_ok(66, 0x1000)


# ------------------------------------------------------------------------------------------------ under the sanitizers
def test_the_index_arithmetic_and_the_mirror_under_asan_ubsan(tmp_path):
    exe = tmp_path / "linear_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "rlap_amd", "csrc"),
                           "-I", os.path.join(ROOT, "tests", "csrc"), "-o", str(exe), os.path.join(ROOT, "tests", "csrc", "linear_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_linear_act": "h x M Fin Fout w b act alpha flags y info",
    "rlap_linear_act_backward": "h x w y gy M Fin Fout act alpha flags gx gw gb info",
}
ARENA = 4321


def f32_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


def fill(addr, count, value):
    out = ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))
    for i in range(count):
        out[i] = value


class LinearStub(StubLib):
    """Records both exports; the forward writes y = 2; the backward gx = 3, gw = 4, gb = 5 where it is asked for them."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        status = self.statuses.pop(0) if self.statuses else self.status
        M, Fin, Fout = a["M"], a["Fin"], a["Fout"]
        rec = {k: a[k] for k in ("M", "Fin", "Fout", "act", "alpha", "flags")}
        rec["x"], rec["w"] = f32_at(a["x"], M * Fin), f32_at(a["w"], Fin * Fout)
        if name.endswith("backward"):
            rec["y"], rec["gy"] = f32_at(a["y"], M * Fout), f32_at(a["gy"], M * Fout)
            rec["asked"] = tuple(k for k in ("gx", "gw", "gb") if a[k])
        else:
            rec["b"] = f32_at(a["b"], Fout) if a["b"] else None
        self.calls.append((name, rec))
        if status:
            return status
        if name.endswith("backward"):
            for key, count, v in (("gx", M * Fin, 3.0), ("gw", Fin * Fout, 4.0), ("gb", Fout, 5.0)):
                if a[key]:
                    fill(a[key], count, v)
        else:
            fill(a["y"], M * Fout, 2.0)
        info = a["info"]._obj
        info.rows, info.fin, info.fout, info.parts, info.arena_bytes, info.host_syncs = M, Fin, Fout, 7, ARENA, 0
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, LinearStub())


def feats(*shape, shift=0.0):
    return torch.arange(int(np.prod(shape)), dtype=torch.float32).reshape(*shape) / 4.0 - 1.0 + shift


def test_arguments_of_the_forward_export(lib):
    x, w, b = feats(5, 3), feats(3, 2, shift=0.5), feats(2, shift=0.25)
    y = ops.linear_act(x, w, b, act="elu", alpha=0.5)
    (name, c), = lib.exports()
    assert name == "rlap_linear_act"
    assert (c["M"], c["Fin"], c["Fout"], c["act"], c["alpha"], c["flags"]) == (5, 3, 2, 2, 0.5, 0)
    assert c["x"] == x.reshape(-1).tolist() and c["w"] == w.reshape(-1).tolist() and c["b"] == b.tolist()
    assert y.shape == (5, 2) and y.dtype == torch.float32 and bool((y == 2).all()) and not y.requires_grad
    assert ops.last_stats == {"rows": 5, "fin": 3, "fout": 2, "parts": 7, "arena_bytes": ARENA, "host_syncs": 0}


def test_defaults_layers_and_the_out_in_layout(lib):
    x, w = feats(2, 5, 3), feats(4, 3)
    y = ops.linear_act(x, w, weight_layout="out_in")
    (_, c), = lib.exports()
    assert (c["M"], c["Fin"], c["Fout"], c["act"], c["alpha"], c["flags"], c["b"]) == (10, 3, 4, 0, 1.0, 1, None)
    assert c["w"] == w.reshape(-1).tolist()                                # as it lies: no transposed copy
    assert y.shape == (2, 5, 4)
    assert (ops.LINEAR_ACT, ops.LINEAR_LAYOUT) == ({"none": 0, "relu": 1, "elu": 2}, {"in_out": 0, "out_in": 1})
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "enum { RLAP_LINEAR_WEIGHT_OUT_IN = 1 };" in hdr
    assert "enum { RLAP_LINEAR_ACT_NONE = 0, RLAP_LINEAR_ACT_RELU = 1, RLAP_LINEAR_ACT_ELU = 2 };" in hdr


def test_non_contiguous_inputs_are_packed(lib):
    x = feats(3, 5).t()          # (5, 3), strided
    ops.linear_act(x, feats(3, 2))
    (_, c), = lib.exports()
    assert c["x"] == x.contiguous().reshape(-1).tolist() and (c["M"], c["Fin"]) == (5, 3)


X, W = torch.zeros(5, 3), torch.zeros(3, 2)
BAD = [
    (torch.zeros(5, 3, dtype=torch.float64), W, {}),                           # dtype
    (X, torch.zeros(3, 2, dtype=torch.float16), {}),
    (torch.zeros(5, 3, dtype=torch.int64), W, {}),
    (torch.zeros(3), W, {}),                                                   # rank
    (torch.zeros(1, 1, 5, 3), W, {}),
    (X, torch.zeros(3), {}),
    (X, torch.zeros(1, 3, 2), {}),
    ([[0.0] * 3] * 5, W, {}),                                                  # not a tensor
    (X, [[0.0] * 2] * 3, {}),
    (X, torch.zeros(4, 2), {}),                                                # Fin differs
    (X, torch.zeros(3, 2), {"weight_layout": "out_in"}),
    (torch.zeros(0, 3), W, {}),                                                # no row
    (torch.zeros(0, 5, 3), W, {}),
    (torch.zeros(5, 513), torch.zeros(513, 2), {}),                            # F > 512
    (X, torch.zeros(3, 513), {}),
    (X, torch.zeros(513, 3), {"weight_layout": "out_in"}),
    (torch.zeros(5, 0), torch.zeros(0, 2), {}),                                # no column
    (X, torch.zeros(3, 0), {}),
    (X, W, {"act": "prelu"}),                                                  # act
    (X, W, {"act": "gelu"}),
    (X, W, {"act": None}),
    (X, W, {"act": 1}),
    (X, W, {"alpha": 0.0}),                                                    # alpha <= 0, not finite, not a number
    (X, W, {"alpha": -1.0}),
    (X, W, {"alpha": float("nan")}),
    (X, W, {"alpha": float("inf")}),
    (X, W, {"alpha": "1"}),
    (X, W, {"alpha": True}),
    (X, W, {"alpha": 0.0, "act": "relu"}),                                     # (checked whatever act is)
    (X, W, {"bias": torch.zeros(3)}),                                          # a bias of the wrong length, rank, dtype or device
    (X, W, {"bias": torch.zeros(1, 2)}),
    (X, W, {"bias": torch.zeros(2, dtype=torch.float64)}),
    (X, W, {"bias": torch.zeros(2, device="meta")}),
    (X, W, {"bias": [0.0, 0.0]}),
    (X, torch.zeros(3, 2, device="meta"), {}),                                 # the weight on another device
    (X, W, {"weight_layout": "io"}),                                           # layout
    (X, W, {"weight_layout": None}),
]


@pytest.mark.parametrize("x,w,kw", BAD)
def test_bad_arguments_raise_value_error_before_any_call(lib, monkeypatch, x, w, kw):
    def reached(*args, **kwargs):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    with pytest.raises(ValueError):
        ops.linear_act(x, w, **kw)
    assert lib.exports() == []


def test_the_ends_of_the_ranges_are_inside(lib):
    ops.linear_act(torch.zeros(1, 512), torch.zeros(512, 512), torch.zeros(512), act="elu", alpha=1e-300)
    ops.linear_act(torch.zeros(1, 1), torch.zeros(1, 1))
    (_, c), (_, d) = lib.exports()
    assert (c["M"], c["Fin"], c["Fout"], c["alpha"]) == (1, 512, 512, 1e-300) and (d["M"], d["Fin"], d["Fout"]) == (1, 1, 1)


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (7, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    before = ops.last_stats
    with pytest.raises(exc, match=f"status {status}"):
        ops.linear_act(feats(4, 2), feats(2, 2))
    assert ops.last_stats is before


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.linear_act(feats(4, 2), feats(2, 2))
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_linear_act")
    assert names[i:i + 4] == ["rlap_linear_act", "rlap_workspace_needed", "rlap_set_workspace", "rlap_linear_act"]
    assert lib.calls[i + 2][1]["ws_bytes"] >= 1 << 20


@pytest.mark.parametrize("need", [("x", "w", "b"), ("x",), ("w",), ("b",), ("w", "b"), ("x", "w")])
def test_autograd_asks_for_the_required_gradients_alone(lib, need):
    x = feats(2, 4, 3).requires_grad_("x" in need)
    w = feats(2, 3, shift=0.5).requires_grad_("w" in need)
    b = feats(2, shift=0.25).requires_grad_("b" in need)
    y = ops.linear_act(x, w, b, act="relu", weight_layout="out_in")
    assert y.requires_grad and y.shape == (2, 4, 2)
    gy = feats(2, 4, 2, shift=3.0)
    y.backward(gy)
    (fname, f), (bname, c) = lib.exports()
    assert (fname, bname) == ("rlap_linear_act", "rlap_linear_act_backward")
    assert (c["M"], c["Fin"], c["Fout"], c["act"], c["alpha"], c["flags"]) == (8, 3, 2, 1, 1.0, 1)
    assert c["x"] == x.detach().reshape(-1).tolist() and c["w"] == w.detach().reshape(-1).tolist()
    assert c["y"] == [2.0] * 16 and c["gy"] == gy.reshape(-1).tolist()              # the forward's y, saved
    assert c["asked"] == tuple(k for k, n in (("gx", "x"), ("gw", "w"), ("gb", "b")) if n in need)
    for t, n, v in ((x, "x", 3.0), (w, "w", 4.0), (b, "b", 5.0)):
        if n in need:
            assert t.grad.shape == t.shape and t.grad.dtype == torch.float32 and bool((t.grad == v).all())
        else:
            assert t.grad is None
    assert ops.last_stats["rows"] == 8 and ops.last_stats["host_syncs"] == 0


def test_no_bias_no_bias_gradient(lib):
    x = feats(4, 3).requires_grad_(True)
    ops.linear_act(x, feats(3, 2)).sum().backward()
    assert lib.exports()[1][1]["asked"] == ("gx",)


def test_no_graph_is_recorded_without_requires_grad(lib):
    assert not ops.linear_act(feats(4, 3), feats(3, 2)).requires_grad
    x = feats(4, 3).requires_grad_(True)
    with torch.no_grad():
        assert not ops.linear_act(x, feats(3, 2)).requires_grad
    assert [c[0] for c in lib.exports()] == ["rlap_linear_act"] * 2


def test_linear_info_layout(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_linear_info", "LinearInfo")
    assert [f for f, _ in _lib.LinearInfo._fields_] == ["rows", "fin", "fout", "parts", "arena_bytes", "host_syncs", "pad"]


def test_exports_are_declared():
    assert {"rlap_linear_act", "rlap_linear_act_backward"} <= set(_lib.EXPORTS)
    api = open(os.path.join(ROOT, "rlap_amd", "csrc", "rlap_api.hip")).read()
    check = api[api.index("int linear_check("):api.index("int rlap_linear_act(")]
    assert all(s in check for s in ("linear::flags_ok(flags)", "linear::alpha_ok(alpha)", "linear::act_ok(act)", "linear::features_ok(Fout)"))


# ------------------------------------------------------------------------------------------------ the adapters
def test_snapshot_linear_loads_a_torch_linear_state_dict(lib):
    ref = torch.nn.Linear(3, 2)
    m = adapters.SnapshotLinear(3, 2, act="elu", alpha=0.5)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    m.load_state_dict(ref.state_dict())
    m(feats(4, 3))
    (_, c), = lib.exports()
    assert c["w"] == ref.weight.detach().reshape(-1).tolist() and c["b"] == ref.bias.detach().tolist()
    assert (c["flags"], c["act"], c["alpha"], c["Fin"], c["Fout"]) == (1, 2, 0.5, 3, 2)
    nb = adapters.SnapshotLinear(3, 2, bias=False)
    nb.load_state_dict(torch.nn.Linear(3, 2, bias=False).state_dict())
    assert nb.bias is None and list(nb.state_dict()) == ["weight"]


def test_snapshot_linear_initialises_as_torch_linear():
    torch.manual_seed(5)
    ref = torch.nn.Linear(7, 4)
    torch.manual_seed(5)
    m = adapters.SnapshotLinear(7, 4)
    assert torch.equal(m.weight, ref.weight) and torch.equal(m.bias, ref.bias)
    with pytest.raises(ValueError):
        adapters.SnapshotLinear(3, 2, act="prelu")


def test_mlp_and_projection_head_are_two_calls_the_first_fused(lib):
    adapters.SnapshotMLP(3, 4, 2)(feats(2, 5, 3))
    adapters.ProjectionHead(3, 4)(feats(5, 3))
    (_, a), (_, b), (_, c), (_, d) = lib.exports()
    assert [(r["M"], r["Fin"], r["Fout"], r["act"], r["flags"]) for r in (a, b, c, d)] == [(10, 3, 4, 1, 1), (10, 4, 2, 0, 1), (5, 3, 4, 2, 1), (5, 4, 3, 0, 1)]
    assert b["x"] == [2.0] * 40                                               # the second call reads the first's result
    head = adapters.ProjectionHead(8, 4)
    assert (head.fc1.in_features, head.fc1.out_features, head.fc2.in_features, head.fc2.out_features) == (8, 4, 4, 8)


def test_the_dense_keyword_defaults_to_torch(lib):
    torch.manual_seed(3)
    old = adapters.SnapshotGINEncoder(3, 4, 2)
    torch.manual_seed(3)
    new = adapters.SnapshotGINEncoder(3, 4, 2, dense="torch")
    assert isinstance(old.layers[0].nn, torch.nn.Sequential) and all(torch.equal(p, q) for p, q in zip(old.parameters(), new.parameters()))
    dev = adapters.SnapshotGINEncoder(3, 4, 2, dense="device")
    assert isinstance(dev.layers[1].nn, adapters.SnapshotMLP)
    g2l = adapters.SnapshotG2LEncoder(3, 4, 1, dense="device")
    assert isinstance(g2l.head_linear, adapters.SnapshotLinear) and isinstance(g2l.layers[0].nn, adapters.SnapshotMLP)
    assert isinstance(adapters.SnapshotG2LEncoder(3, 4, 1).head_linear, torch.nn.Linear)
    assert adapters.SnapshotGCNConv(3, 2).dense == "torch"
    for cls, args in ((adapters.SnapshotGCNConv, (3, 2)), (adapters.SnapshotGINEncoder, (3, 4, 1)), (adapters.SnapshotG2LEncoder, (3, 4, 1))):
        with pytest.raises(ValueError):
            cls(*args, dense="rocblas")


def test_gcn_conv_with_the_device_product_calls_linear_act(lib):
    class Holder:
        def propagate(self, x, transpose=False):
            return torch.stack([x, x])
    conv = adapters.SnapshotGCNConv(3, 2, dense="device")
    out = conv(feats(4, 3), Holder())
    (name, c), = lib.exports()
    assert name == "rlap_linear_act" and (c["M"], c["Fin"], c["Fout"], c["act"], c["flags"], c["b"]) == (4, 3, 2, 0, 0, None)
    assert c["w"] == conv.weight.detach().reshape(-1).tolist() and out.shape == (2, 4, 2)
