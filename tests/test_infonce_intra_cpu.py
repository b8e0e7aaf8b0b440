"""The InfoNCE calls with intraview negatives (ops.info_nce / ops.info_nce_pair with intraview="masked" | "all", rlap_infonce_intra and
its three kin) without a GPU:

  * the rule -- the host mirror (tests/csrc/infonce_intra_mirror.cc, every value from rlap_amd/csrc/rlap_infonce.h, contraction off)
    against a float64 torch restatement of the sampler's concatenation with GCL's InfoNCE ("masked") and the reference's
    InfoNCEBatched ("all") and its autograd, one-way and pair, both `positive` settings, tau in {1/32, 0.4, 2}; the pair against the
    mean of two one-way calls; N = 1; the invariances;
  * the index arithmetic of both streams in a stand-alone program under -fsanitize=address,undefined, exhaustively for N <= 300;
  * the Python -> C mapping of the four exports on a stub library, "none" reaching the plain exports alone, adapters.NodeContrast.

The bounds are four times the largest differences measured with these inputs (DESIGN 4.24 has the figures), the margin
tests/test_infonce_cpu.py took for float32 chains of length F.  Measured here, mirror against the restatement at the four large
shapes: loss 5.03e-8 relative, gradients 3.78e-6 of the largest entry.  At (1, 3) and (2, 5) a "masked" loss and its gradients
vanish in exact arithmetic (one row has no negative at all, and at tau = 1/32 the single negative of two rows weighs e^-32), so there
the differences are taken as a share of max(|value|, 1): loss 1.19e-7, gradients 6.21e-7.  Pair mirror against two one-way mirror
calls: gradients 1.86e-6 of the largest entry at the large shapes (one float32 chain of folded weights against the float64 sum of two
float32 chains), 3.04e-7 of max(|value|, 1) at the two small ones; Z and Zc within N 2^-52 relative (the same float64 terms in another
order); the loss differed in NO bit, so its bound is test_infonce_pair_cpu.py's PAIR_LOSS_ABS(N) = (N + 256) 2^-52 with 2 N terms
in either sum: (2 N + 256) 2^-52, absolute.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import infonce_intra_mirror as xm
import infonce_mirror as im
from rlap_amd import _lib, adapters, ops
from util import StubLib, f64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOSS_BOUND = 4 * 5.03e-8           # against the restatement, relative to the loss
GRAD_BOUND = 4 * 3.78e-6           # against the restatement, relative to the largest gradient entry
SMALL_LOSS_BOUND = 4 * 1.19e-7     # N <= 2: relative to max(|loss|, 1)
SMALL_GRAD_BOUND = 4 * 6.21e-7     # N <= 2: relative to max(largest gradient entry, 1)
PAIR_GRAD_BOUND = 4 * 1.86e-6      # pair against two one-way mirror calls, relative to the largest gradient entry
SMALL_PAIR_GRAD_BOUND = 4 * 3.04e-7     # the same at N <= 2, of max(largest entry, 1)
VARIANTS = ("masked", "all")


def pair_loss_abs(n):
    return (2 * n + 256) * 2.0 ** -52


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return xm.build(tmp_path_factory.mktemp("infonce_intra"))


@pytest.fixture(scope="module")
def mirror1(tmp_path_factory):
    return im.build(tmp_path_factory.mktemp("infonce_one"))


def views(n, f, seed):
    """Two float32 views whose positives have cosine about 0.3 (as tests/test_infonce_cpu.py)."""
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((n, f)).astype(np.float32)
    b = (0.3 * a + rng.standard_normal((n, f))).astype(np.float32)
    return a, b


# ------------------------------------------------------------------------------------------------ the rule
SHAPES = [(33, 3), (65, 33), (300, 100), (129, 512), (1, 3), (2, 5)]
RULE = [(n, f, positive, tau) for n, f in SHAPES for positive in ("scaled", "raw") for tau in (1.0 / 32.0, 0.4, 2.0)]
G_UP = 0.75


@pytest.fixture(scope="module")
def runs(mirror):
    cache = {}

    def get(n, f, positive, tau, variant, pair):
        key = (n, f, positive, tau, variant, pair)
        if key not in cache:
            a, b = views(n, f, 1000 + n)
            cache[key] = (a, b, xm.run(mirror, a, b, tau, positive, variant, g=G_UP, pair=pair))
        return cache[key]
    get.lib = mirror
    return get


def shares(n, value, diff):
    """A difference as a share of the value it belongs to; at N <= 2, where the value may vanish, of max(|value|, 1)."""
    return diff / (max(abs(value), 1.0) if n <= 2 else abs(value))


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,f,positive,tau", RULE)
def test_mirror_against_the_float64_restatement(runs, n, f, positive, tau, variant, pair):
    a, b, m = runs(n, f, positive, tau, variant, pair)
    loss, ga, gb = xm.restatement(a, b, tau, positive, variant, g=G_UP, pair=pair)
    rel = shares(n, loss, abs(m["loss"] - loss))
    gmax = max(np.abs(ga).max(), np.abs(gb).max())
    grel = shares(n, gmax, max(np.abs(m["ga"] - ga).max(), np.abs(m["gb"] - gb).max()))
    print(f"n={n} F={f} {positive} tau={tau} {variant} pair={pair}: loss {loss:.6g} rel {rel:.3g}, gradients rel {grel:.3g}")
    if n > 2:
        assert 0.05 < abs(loss) < 50.0                            # the relative error is meaningful
    assert rel <= (LOSS_BOUND if n > 2 else SMALL_LOSS_BOUND)
    assert grel <= (GRAD_BOUND if n > 2 else SMALL_GRAD_BOUND)
    assert np.isfinite(m["rows"]).all() and abs(-m["rows"].mean() - loss) <= (LOSS_BOUND if n > 2 else SMALL_LOSS_BOUND) * max(abs(loss), 1.0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,f,positive,tau", RULE)
def test_pair_mirror_against_the_mean_of_two_one_way_calls(runs, n, f, positive, tau, variant):
    a, b, p = runs(n, f, positive, tau, variant, True)
    _, _, m1 = runs(n, f, positive, tau, variant, False)
    m2 = xm.run(runs.lib, b, a, tau, positive, variant, g=G_UP)
    loss = 0.5 * (m1["loss"] + m2["loss"])
    ga = 0.5 * (m1["ga"].astype(np.float64) + m2["gb"])
    gb = 0.5 * (m1["gb"].astype(np.float64) + m2["ga"])
    assert p["sii"].tobytes() == m1["sii"].tobytes() == m2["sii"].tobytes()        # fmaf(x, y, acc) == fmaf(y, x, acc)
    gmax = max(np.abs(ga).max(), np.abs(gb).max())
    dl = abs(p["loss"] - loss)
    grel = shares(n, gmax, max(np.abs(p["ga"] - ga).max(), np.abs(p["gb"] - gb).max()))
    zrel = (np.abs(p["z"] - np.stack([m1["z"], m2["z"]])) / p["z"]).max()
    print(f"n={n} F={f} {positive} tau={tau} {variant}: loss diff {dl:.3g}, gradients rel {grel:.3g}, Z and Zc rel {zrel:.3g}")
    assert dl <= pair_loss_abs(n)
    assert grel <= (PAIR_GRAD_BOUND if n > 2 else SMALL_PAIR_GRAD_BOUND)
    assert zrel <= 2 * n * 2.0 ** -52


@pytest.mark.parametrize("positive", ["scaled", "raw"])
@pytest.mark.parametrize("pair", [False, True])
def test_one_row_masked_gives_the_bits_of_the_plain_mirror(mirror, mirror1, positive, pair):
    """With N = 1 the masked intraview set is empty, and 0 + x = x: every result is the plain call's."""
    a, b = views(1, 3, 5)
    m = xm.run(mirror, a, b, 0.4, positive, "masked", g=1.0, pair=pair)
    q = im.run(mirror1, a, b, 0.4, positive, g=1.0)
    assert m["sii"].tobytes() == q["sii"].tobytes()
    if not pair:
        for key in ("loss", "z", "rows", "ga", "gb"):
            assert np.asarray(m[key]).tobytes() == np.asarray(q[key]).tobytes(), key
    else:
        assert m["z"][0].tobytes() == m["z"][1].tobytes() == q["z"].tobytes() and m["rows"][0].tobytes() == q["rows"].tobytes()
        assert np.float64(m["loss"]).tobytes() == np.float64(q["loss"]).tobytes()
    w = xm.run(mirror, a, b, 0.4, positive, "all", pair=pair)
    assert (w["z"] > m["z"]).all()                                # "all" counts e_ii, which is 1 up to a few roundings
    assert np.abs(w["z"] - m["z"] - 1.0).max() < 1e-5


@pytest.mark.parametrize("variant", VARIANTS)
def test_the_variants_differ_by_the_diagonal_term_alone(mirror, variant):
    a, b = views(65, 33, 5)
    m, w = xm.run(mirror, a, b, 0.4, "scaled", "masked"), xm.run(mirror, a, b, 0.4, "scaled", "all")
    assert m["sii"].tobytes() == w["sii"].tobytes()
    assert np.abs(w["z"] - m["z"] - 1.0).max() < 1e-5
    s, r = xm.run(mirror, a, b, 0.4, "scaled", variant), xm.run(mirror, a, b, 0.4, "raw", variant)
    assert s["z"].tobytes() == r["z"].tobytes()
    assert np.abs(r["rows"] - (s["rows"] - (1.0 / 0.4 - 1.0) * s["sii"].astype(np.float64))).max() < 1e-12


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_the_row_tiling_changes_no_bit(mirror, variant, pair):
    a, b = views(70, 9, 3)
    base = xm.run(mirror, a, b, 0.4, "raw", variant, g=1.0, pair=pair, block_rows=32)
    for block in (1, 7, 128):
        other = xm.run(mirror, a, b, 0.4, "raw", variant, g=1.0, pair=pair, block_rows=block)
        for key in ("loss", "z", "rows", "ga", "gb", "sii"):
            assert np.asarray(base[key]).tobytes() == np.asarray(other[key]).tobytes(), (key, block)


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("f,pad", [(3, 1), (31, 1), (32, 32), (33, 31)])
def test_zero_feature_columns_change_no_bit(mirror, f, pad, pair):
    a, b = views(65, f, 11)
    wide = lambda x: np.concatenate([x, np.zeros((x.shape[0], pad), dtype=np.float32)], axis=1)
    for variant in VARIANTS:
        m = xm.run(mirror, a, b, 0.4, "scaled", variant, g=1.0, pair=pair)
        w = xm.run(mirror, wide(a), wide(b), 0.4, "scaled", variant, g=1.0, pair=pair)
        for key in ("loss", "z", "rows"):
            assert np.asarray(m[key]).tobytes() == np.asarray(w[key]).tobytes(), key
        for key in ("ga", "gb"):
            assert m[key].tobytes() == w[key][:, :f].tobytes() and not w[key][:, f:].any(), key


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("variant", VARIANTS)
def test_a_zero_row_gives_finite_values(mirror, variant, pair):
    a, b = views(40, 5, 13)
    a[3] = 0.0
    b[17] = 0.0
    m = xm.run(mirror, a, b, 0.4, "raw", variant, g=1.0, pair=pair)
    for key in ("loss", "z", "rows", "ga", "gb"):
        assert np.isfinite(np.asarray(m[key])).all(), key
    assert m["sii"][3] == 0.0 and m["sii"][17] == 0.0
    loss, _, _ = xm.restatement(a, b, 0.4, "raw", variant, pair=pair)
    assert abs(m["loss"] - loss) <= LOSS_BOUND * abs(loss)


def test_the_mirror_refuses_what_the_library_refuses(mirror):
    assert [mirror.intra_ok(v) for v in (-1, 0, 1, 2, 3)] == [0, 0, 1, 1, 0]
    assert mirror.intra_member(1, 4, 4) == 0 and mirror.intra_member(1, 4, 5) == 1 and mirror.intra_member(2, 4, 4) == 1
    assert mirror.intra_z_parts(300) == 2 * 10 and mirror.intra_z_parts(169343) == 2


# ------------------------------------------------------------------------------------------------ the index arithmetic, under the sanitizers
def test_the_index_arithmetic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "infonce_intra_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "infonce_intra_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "300 sizes, 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ the entry points on a stub
PLAIN = {
    "rlap_infonce": "h a b n F tau flags loss rows z info",
    "rlap_infonce_backward": "h a b n F tau flags z g ga gb info",
    "rlap_infonce_pair": "h a b n F tau flags loss rows z info",
    "rlap_infonce_pair_backward": "h a b n F tau flags z g ga gb info",
}
SIGS = dict(PLAIN)
SIGS.update({
    "rlap_infonce_intra": "h a b n F tau flags intraview loss rows z info",
    "rlap_infonce_intra_backward": "h a b n F tau flags intraview z g ga gb info",
    "rlap_infonce_pair_intra": "h a b n F tau flags intraview loss rows z info",
    "rlap_infonce_pair_intra_backward": "h a b n F tau flags intraview z g ga gb info",
})
ARENA = 9876


def f32_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


class IntraStub(StubLib):
    """Records the eight exports.  Forward: loss = 1.5, rows = -1, z = 2 (pair: the second list rows = -3, z = 5); backward: ga = 3,
    gb = 4."""

    def __init__(self):
        super().__init__(SIGS)

    def export(self, name, a):
        n, F = a["n"], a["F"]
        pair = "pair" in name
        lists = 2 if pair else 1
        rec = {k: a.get(k) for k in ("n", "F", "tau", "flags", "intraview")}
        rec["a"], rec["b"] = f32_at(a["a"], n * F), f32_at(a["b"], n * F)
        back = name.endswith("backward")
        if back:
            rec["z"], rec["g"] = f64_at(a["z"], lists * n), f64_at(a["g"], 1)
        self.calls.append((name, rec))
        if self.status:
            return self.status
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
    return stub_ops(monkeypatch, IntraStub())


def feats(n, f, shift=0.0):
    return (torch.arange(n * f, dtype=torch.float32).reshape(n, f) / 4.0 - 1.0 + shift)


CALLS = [(ops.info_nce, "rlap_infonce", 1), (ops.info_nce_pair, "rlap_infonce_pair", 2)]


@pytest.mark.parametrize("call,stem,lists", CALLS)
@pytest.mark.parametrize("variant,value", [("masked", 1), ("all", 2)])
@pytest.mark.parametrize("positive,flags", [("scaled", 0), ("raw", 1)])
def test_arguments_of_the_forward_exports(lib, call, stem, lists, variant, value, positive, flags):
    a, b = feats(5, 3), feats(5, 3, 0.5)
    loss, rows = call(a, b, tau=0.5, positive=positive, return_rows=True, intraview=variant)
    (name, c), = lib.exports()
    assert name == stem + "_intra"
    assert (c["n"], c["F"], c["tau"], c["flags"], c["intraview"]) == (5, 3, 0.5, flags, value)
    assert c["a"] == a.reshape(-1).tolist() and c["b"] == b.reshape(-1).tolist()
    assert loss.dim() == 0 and loss.dtype == torch.float64 and float(loss) == 1.5
    assert rows.shape == ((2, 5) if lists == 2 else (5,)) and bool((rows.reshape(lists, 5)[0] == -1).all())
    assert ops.last_stats["arena_bytes"] == ARENA and ops.last_stats["host_syncs"] == 0 and not loss.requires_grad


@pytest.mark.parametrize("call,stem,lists", CALLS)
@pytest.mark.parametrize("variant,value", [("masked", 1), ("all", 2)])
def test_autograd_carries_the_variant_to_the_backward_export(lib, call, stem, lists, variant, value):
    a, b = feats(4, 3).requires_grad_(True), feats(4, 3, 0.25).requires_grad_(True)
    loss = call(a, b, tau=0.5, positive="raw", intraview=variant)
    (2.5 * loss).backward()
    (fname, f), (bname, c) = lib.exports()
    assert (fname, bname) == (stem + "_intra", stem + "_intra_backward")
    assert (c["n"], c["F"], c["tau"], c["flags"], c["intraview"]) == (4, 3, 0.5, 1, value) == (f["n"], f["F"], f["tau"], f["flags"], f["intraview"])
    assert c["a"] == a.detach().reshape(-1).tolist() and c["b"] == b.detach().reshape(-1).tolist()
    assert c["z"] == [2.0] * 4 + [5.0] * 4 * (lists - 1) and c["g"] == [2.5]
    assert bool((a.grad == 3).all()) and bool((b.grad == 4).all()) and a.grad.dtype == torch.float32


@pytest.mark.parametrize("call,stem,lists", CALLS)
def test_none_reaches_the_plain_exports_alone_with_their_arguments(lib, call, stem, lists):
    a, b = feats(4, 3).requires_grad_(True), feats(4, 3, 0.25)
    call(a, b, tau=0.5).backward()
    call(a, b, tau=0.5, intraview="none")
    names = [c[0] for c in lib.exports()]
    assert names == [stem, stem + "_backward", stem]
    assert all(c[1]["intraview"] is None for c in lib.exports())          # the plain signatures have no such argument
    assert set(names) <= set(PLAIN)


@pytest.mark.parametrize("bad", ["both", "", None, True, 1, 2, "MASKED", b"all"])
def test_bad_intraview_values_raise_value_error_before_any_call(lib, monkeypatch, bad):
    def reached(*args, **kw):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    for call in (ops.info_nce, ops.info_nce_pair):
        with pytest.raises(ValueError):
            call(feats(4, 3), feats(4, 3), intraview=bad)
    assert lib.exports() == []


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    for call in (ops.info_nce, ops.info_nce_pair):
        with pytest.raises(exc, match=f"status {status}"):
            call(feats(4, 2), feats(4, 2), intraview="all")


def test_exports_are_declared():
    new = ["rlap_infonce_intra", "rlap_infonce_intra_backward", "rlap_infonce_pair_intra", "rlap_infonce_pair_intra_backward"]
    assert set(new) <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    for name in new:
        assert f"int {name}(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview," in hdr
    assert "enum { RLAP_INFONCE_INTRA_MASKED = 1, RLAP_INFONCE_INTRA_ALL = 2 };" in hdr
    assert (_lib.INFONCE_INTRA_MASKED, _lib.INFONCE_INTRA_ALL) == (1, 2)
    lib = _lib.load()
    for name, info in (("rlap_infonce_intra", _lib.InfonceInfo), ("rlap_infonce_pair_intra", _lib.InfoncePairInfo)):
        for fn in (getattr(lib, name), getattr(lib, name + "_backward")):
            assert fn.argtypes[-1]._type_ is info and fn.argtypes[7] is ctypes.c_int and fn.argtypes[6] is ctypes.c_int
    assert len(lib.rlap_infonce_intra.argtypes) == len(lib.rlap_infonce.argtypes) + 1
    assert len(lib.rlap_infonce_pair_intra_backward.argtypes) == len(lib.rlap_infonce_pair_backward.argtypes) + 1


# ------------------------------------------------------------------------------------------------ the adapter
@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("setting,value", [(True, 1), ("masked", 1), ("all", 2)])
def test_node_contrast_maps_the_switch(lib, pair, setting, value):
    h1, h2 = feats(4, 3).requires_grad_(True), feats(4, 3, 0.5).requires_grad_(True)
    contrast = adapters.NodeContrast(tau=0.5, pair=pair, intraview_negs=setting)
    contrast(h1, h2).backward()
    stem = "rlap_infonce_pair_intra" if pair else "rlap_infonce_intra"
    times = 1 if pair else 2
    assert sorted(c[0] for c in lib.exports()) == [stem] * times + [stem + "_backward"] * times
    assert all(c[1]["intraview"] == value and c[1]["flags"] == 1 and c[1]["tau"] == 0.5 for c in lib.exports())   # "raw" by default
    assert bool((h1.grad == (3 if pair else 3 + 4)).all())                # (the stub's ga, and gb of the swapped call)


@pytest.mark.parametrize("pair", [False, True])
def test_node_contrast_false_is_the_plain_loss(lib, pair):
    for contrast in (adapters.NodeContrast(tau=0.5, pair=pair), adapters.NodeContrast(tau=0.5, pair=pair, intraview_negs=False)):
        assert contrast.intraview == "none"
        contrast(feats(4, 3), feats(4, 3, 0.5))
    assert {c[0] for c in lib.exports()} == {"rlap_infonce_pair" if pair else "rlap_infonce"}


@pytest.mark.parametrize("bad", ["both", None, 1, 0, 2.0, "ALL"])
def test_node_contrast_refuses_a_bad_switch_before_any_call(lib, bad):
    with pytest.raises(ValueError):
        adapters.NodeContrast(intraview_negs=bad)
    assert lib.exports() == []
