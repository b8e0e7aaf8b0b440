"""The fused graph-to-local losses (ops.g2l_jsd / ops.g2l_bootstrap, rlap_g2l_*) without a GPU:

  * the rule -- the host mirror (tests/csrc/g2l_mirror.cc, every value from rlap_amd/csrc/rlap_g2l.h, contraction off) against a
    float64 torch restatement of the reference's JSD.compute with the sampler's masks and of BootstrapLatent, and their autograd;
    softplus at the ends of its branches; what is left out of the sums; the order's invariances;
  * the index arithmetic of the header in a stand-alone program under -fsanitize=address,undefined, exhaustively for N <= 300;
  * the Python -> C mapping of the four exports on a stub library, the layout of rlap_g2l_info, the two adapters.

The bounds of the first group are four times the largest differences measured with these inputs (DESIGN 4.17 has the figures): the
rule's error is that of float32 chains of length F and of a float32 exponential, a property of the formats and not of the seed.
Measured here: JSD loss 6.12e-8 relative, JSD gradients 1.24e-6 of the largest entry (F = 512); bootstrap loss 4.92e-8 of its scale,
bootstrap gradients 8.57e-8 of the largest entry.  The entries of h are 0.5 N(0, 1) and those of g N(0, 1): the JSD losses are then
of order 1 and do not cancel.  The bootstrap's cosines of such inputs do cancel (a loss of 0.018 from 129 terms of size 0.04 at F = 512), so
its error is taken relative to sum_i |c_i| / G, the size of what is summed, which no cancellation shrinks.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import g2l_mirror as gm
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, f64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JSD_LOSS_BOUND = 4 * 6.12e-8      # relative to the loss
JSD_GRAD_BOUND = 4 * 1.24e-6      # relative to the largest gradient entry
BOOT_LOSS_BOUND = 4 * 4.92e-8     # relative to sum |c_i| / G
BOOT_GRAD_BOUND = 4 * 8.57e-8     # relative to the largest gradient entry
EXPW_BOUND = 4 * 7.63e-8          # tests/test_infonce_cpu.py: expw against float64 exp, relative


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return gm.build(tmp_path_factory.mktemp("g2l"))


def inputs(n, G, f, seed=None):
    """h = 0.5 N(0, 1), g = N(0, 1), neg = 0.5 N(0, 1) (one graph only)."""
    rng = np.random.RandomState(2000 + n if seed is None else seed)
    h = (0.5 * rng.standard_normal((n, f))).astype(np.float32)
    g = rng.standard_normal((G, f)).astype(np.float32)
    neg = (0.5 * rng.standard_normal((n, f))).astype(np.float32) if G == 1 else None
    return h, g, neg


# (N, G, F, table): (300, 5, 100) has an empty graph at the front, in the middle and at the end
SHAPES = [(33, 1, 3, None), (65, 2, 33, "even"), (300, 5, 100, "empty"), (129, 33, 512, "even")]


def table_of(n, G, kind):
    return None if kind is None else gm.table(n, G, kind)


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("n,G,f,kind", SHAPES)
def test_jsd_mirror_against_the_float64_restatement(mirror, n, G, f, kind):
    h, g, neg = inputs(n, G, f)
    t = table_of(n, G, kind)
    m = gm.run_jsd(mirror, h, g, t, neg, gup=0.75)
    loss, gh, gn, gg = gm.restatement("jsd", h, g, t, neg, gup=0.75)
    rel = abs(m["loss"] - loss) / abs(loss)
    pairs = [(m["gh"], gh), (m["gg"], gg)] + ([(m["gneg"], gn)] if neg is not None else [])
    gmax = max(np.abs(w).max() for _, w in pairs)
    grel = max(np.abs(a - w).max() for a, w in pairs) / gmax
    print(f"jsd n={n} G={G} F={f}: loss {loss:.6g} rel {rel:.3g}, gradients rel {grel:.3g}")
    assert 0.05 < abs(loss) < 50.0                                # the relative error is meaningful
    assert rel <= JSD_LOSS_BOUND
    assert grel <= JSD_GRAD_BOUND
    num_neg = n if G == 1 else n * G - n
    assert mirror.g2l_num_neg(n, G) == num_neg
    assert abs((m["neg"].sum() / num_neg - m["pos"].sum() / n) - loss) <= JSD_LOSS_BOUND * abs(loss)


@pytest.mark.parametrize("n,G,f,kind", SHAPES)
def test_bootstrap_mirror_against_the_float64_restatement(mirror, n, G, f, kind):
    h, g, _ = inputs(n, G, f)
    t = table_of(n, G, kind)
    m = gm.run_bootstrap(mirror, h, g, t, gup=0.75)
    loss, gh, _, _ = gm.restatement("bootstrap", h, g, t, gup=0.75)
    scale = np.abs(m["c"]).sum() / G
    rel = abs(m["loss"] - loss) / scale
    grel = np.abs(m["gh"] - gh).max() / np.abs(gh).max()
    print(f"bootstrap n={n} G={G} F={f}: loss {loss:.6g} scale {scale:.3g} rel to scale {rel:.3g}, rel to |loss| "
          f"{abs(m['loss'] - loss) / abs(loss):.3g}, gradient rel {grel:.3g}")
    assert scale > 0.05 and np.abs(m["c"]).max() <= 1.0 + 1e-6
    assert rel <= BOOT_LOSS_BOUND
    assert grel <= BOOT_GRAD_BOUND


def test_softplus_at_the_ends_of_its_branches(mirror):
    for s in (0.0, 1e-30, -1e-30, 20.0, -20.0, 21.0, -21.0, 64.0, -64.0, 1e4, -1e4):
        s32 = float(np.float32(s))
        e = math.exp(-abs(s32))
        softplus = lambda x: max(x, 0.0) + math.log1p(e)
        pos, neg = mirror.g2l_pos_term(s), mirror.g2l_neg_term(s)
        # expw's relative error on e, the clamp of the exponent at 64 (exp(-64) = 1.6e-28 where the true e is smaller), and the
        # rounding of the float64 restatement itself
        bound = EXPW_BOUND * e + 2e-28 + 4e-16 * abs(s32) + 1e-16
        assert abs(pos - (math.log(2) - softplus(-s32))) <= bound, (s, pos)
        assert abs(neg - (softplus(s32) - math.log(2))) <= bound, (s, neg)
    # a score of 0 gives exactly 0: no rounded ln 2 is left in a term
    assert mirror.g2l_pos_term(0.0) == 0.0 and mirror.g2l_neg_term(0.0) == 0.0
    # no switch to the identity above 20: softplus(21) - 21 is log1p(exp(-21)) = 7.6e-10, not 0
    assert 7.0e-10 < mirror.g2l_neg_term(21.0) + math.log(2) - 21.0 < 8.0e-10
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert math.isnan(mirror.g2l_pos_term(bad)) and math.isnan(mirror.g2l_neg_term(bad)) and math.isnan(mirror.g2l_sigma(bad))
    assert mirror.g2l_sigma(0.0) == 0.5 and abs(mirror.g2l_sigma(2.0) + mirror.g2l_sigma(-2.0) - 1.0) < 2e-7


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("G", [1, 3])
def test_a_score_that_is_not_finite_gives_a_nan_loss(mirror, G, bad):
    h, g, neg = inputs(40, G, 5, seed=3)
    h[7, 2] = bad
    m = gm.run_jsd(mirror, h, g, None if G == 1 else gm.table(40, G), neg)
    assert math.isnan(m["loss"])
    assert np.isfinite(np.delete(m["pos"], 7)).all() and np.isfinite(np.delete(m["neg"], 7 if G > 1 else [])).all()


# ------------------------------------------------------------------------------------------------ what is left out; order and invariance
@pytest.mark.parametrize("f,pad", [(3, 1), (31, 1), (32, 32), (33, 31)])
@pytest.mark.parametrize("G", [1, 5])
def test_zero_feature_columns_change_no_bit(mirror, G, f, pad):
    h, g, neg = inputs(65, G, f, seed=11)
    t = None if G == 1 else gm.table(65, G, "empty")
    wide = lambda x: None if x is None else np.concatenate([x, np.zeros((x.shape[0], pad), dtype=np.float32)], axis=1)
    m = gm.run_jsd(mirror, h, g, t, neg, gup=1.0)
    w = gm.run_jsd(mirror, wide(h), wide(g), t, wide(neg), gup=1.0)
    for key in ("loss", "pos", "neg"):
        assert np.asarray(m[key]).tobytes() == np.asarray(w[key]).tobytes(), key
    for key in ("gh", "gg") + (("gneg",) if G == 1 else ()):
        assert m[key].tobytes() == w[key][:, :f].tobytes() and not w[key][:, f:].any(), key
    b = gm.run_bootstrap(mirror, h, g, t, gup=1.0)
    bw = gm.run_bootstrap(mirror, wide(h), wide(g), t, gup=1.0)
    assert b["loss"].tobytes() == bw["loss"].tobytes() and b["c"].tobytes() == bw["c"].tobytes()
    assert b["gh"].tobytes() == bw["gh"][:, :f].tobytes() and not bw["gh"][:, f:].any()


@pytest.mark.parametrize("G,extra", [(2, 1), (5, 27), (31, 2), (33, 40)])
def test_graphs_without_nodes_change_no_positive_term(mirror, G, extra):
    """Graphs without nodes appended to the table (and rows to g): every positive term keeps its bits, whichever tile the padding
    of the last graph tile falls in -- a column j >= G and the column g(i) are left out of neg_i, never added as zeros.  The
    NEGATIVE sums legitimately change: an appended graph's summary is a negative of every node (num_neg grows by N per graph), and
    neg_i grows by exactly those terms.  The bootstrap's cosines keep their bits and its loss is the same sum over a larger G."""
    n, f = 70, 9
    h, g, _ = inputs(n, G, f, seed=17)
    t = gm.table(n, G)
    rng = np.random.RandomState(5)
    g2 = np.concatenate([g, rng.standard_normal((extra, f)).astype(np.float32)])
    t2 = np.concatenate([t, np.full(extra, n, dtype=np.int64)])
    m, w = gm.run_jsd(mirror, h, g, t), gm.run_jsd(mirror, h, g2, t2)
    assert m["pos"].tobytes() == w["pos"].tobytes()
    s_new = h.astype(np.float64) @ g2[G:].astype(np.float64).T
    added = (np.logaddexp(0.0, s_new) - math.log(2)).sum(axis=1)
    assert np.abs((w["neg"] - m["neg"]) - added).max() <= 1e-5 * (1.0 + np.abs(added).max()) and np.abs(added).max() > 0.01
    b, bw = gm.run_bootstrap(mirror, h, g, t), gm.run_bootstrap(mirror, h, g2, t2)
    assert b["c"].tobytes() == bw["c"].tobytes() and abs(bw["loss"] * (G + extra) - b["loss"] * G) <= 1e-12 * (1 + abs(b["loss"] * G))


def reg_row(r, hf):
    return (r & 3) + 8 * (r >> 2) + 4 * hf


@pytest.mark.parametrize("v", [0.0, 0.25])
@pytest.mark.parametrize("G", [2, 31, 33, 65])
def test_the_positive_and_the_padding_are_left_out_not_added_as_zeros(mirror, G, v):
    """h = v and g = 1 over four columns make every score exactly 4 v, so every negative term is one value (exactly 0 for
    v = 0) and neg_i is that value added G - 1 times in the header's order: not G times, not 32 times."""
    n = 40
    h = np.full((n, 4), v, dtype=np.float32)
    g = np.ones((G, 4), dtype=np.float32)
    t = gm.table(n, G)
    m = gm.run_jsd(mirror, h, g, t)
    term = mirror.g2l_neg_term(4 * v)
    batch = gm.batch_of(t, n)
    for i in range(n):
        half = [0.0, 0.0]
        for tile in range((G + 31) // 32):
            for hf in (0, 1):
                for r in range(16):
                    j = 32 * tile + reg_row(r, hf)
                    if j < G and j != batch[i]:
                        half[hf] += term
        assert m["neg"][i] == half[0] + half[1], (i, G)
    assert (m["pos"] == mirror.g2l_pos_term(4 * v)).all()
    if v:
        assert abs(m["neg"][0] - (G - 1) * term) < 1e-12 * G and abs(term) > 0.3


@pytest.mark.parametrize("n,G,f", [(65, 1, 33), (300, 5, 20), (70, 40, 9)])
def test_row_tiling_changes_no_bit(mirror, n, G, f):
    """The mirror computes every row on its own, so `block_rows` only changes how rows are grouped and dealt to threads: this pins
    the mirror, not the kernels.  The guard against an order that depends on the grid is the bit-for-bit comparison on the device."""
    h, g, neg = inputs(n, G, f, seed=7)
    t = None if G == 1 else gm.table(n, G, "empty" if G >= 4 else "even")
    base = gm.run_jsd(mirror, h, g, t, neg, gup=1.0, block_rows=32)
    bbase = gm.run_bootstrap(mirror, h, g, t, gup=1.0, block_rows=32)
    for block in (1, 7, 128, 1000):
        other = gm.run_jsd(mirror, h, g, t, neg, gup=1.0, block_rows=block)
        for key in ("loss", "pos", "neg", "gh", "gg") + (("gneg",) if G == 1 else ()):
            assert np.asarray(base[key]).tobytes() == np.asarray(other[key]).tobytes(), (block, key)
        bother = gm.run_bootstrap(mirror, h, g, t, gup=1.0, block_rows=block)
        for key in ("loss", "c", "gh"):
            assert np.asarray(bbase[key]).tobytes() == np.asarray(bother[key]).tobytes(), (block, key)


def test_parts_and_the_map(mirror):
    for n, G, f in ((1, 1, 1), (33, 1, 3), (300, 5, 100), (4245, 128, 32), (169343, 1, 512), (4194304, 1024, 64)):
        p = mirror.g2l_parts(n, G, f)
        tiles = (n + 31) // 32
        assert 1 <= p <= min(tiles, 1024) and mirror.g2l_part_begin(n, G, f, 0) == 0 and mirror.g2l_part_begin(n, G, f, p) == tiles
        assert p == mirror.g2l_parts(n, G, 1)                     # F does not enter today
    assert mirror.g2l_parts(4194304, 1024, 64) == 32 and mirror.g2l_parts(169343, 1, 512) == 1024 and mirror.g2l_parts(4245, 128, 32) == 133
    t = np.array([0, 0, 3, 3, 3, 10, 10], dtype=np.int64)
    assert [mirror.g2l_graph_of(t.ctypes.data, 6, 10, i) for i in range(10)] == [1, 1, 1, 4, 4, 4, 4, 4, 4, 4]
    wide = np.array([0, 1, 1, 2, 2, 2, 2], dtype=np.int64)       # G > N
    assert [mirror.g2l_graph_of(wide.ctypes.data, 6, 2, i) for i in range(2)] == [0, 2]
    assert mirror.g2l_num_neg((1 << 31) - 1, (1 << 31) - 1) == ((1 << 31) - 1) * ((1 << 31) - 2)   # formed in int64


# ------------------------------------------------------------------------------------------------ the index arithmetic, under the sanitizers
def test_the_index_arithmetic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "g2l_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "g2l_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "300"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "300 sizes, 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_g2l_jsd": "h x neg g n F node_ptr G flags loss rows info",
    "rlap_g2l_jsd_backward": "h x neg g n F node_ptr G flags gup gh gneg gg info",
    "rlap_g2l_bootstrap": "h x g n F node_ptr G flags loss rows info",
    "rlap_g2l_bootstrap_backward": "h x g n F node_ptr G flags gup gh info",
}
ARENA = 4321


def f32_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


def i64_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_int64))[:count])


class G2lStub(StubLib):
    """Records the four exports; the forwards write loss = 1.5 and rows = -1; the backwards gh = 3, gneg = 4, gg = 5."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        status = self.statuses.pop(0) if self.statuses else self.status
        n, F, G = a["n"], a["F"], a["G"]
        jsd, back = "jsd" in name, name.endswith("backward")
        rec = {k: a[k] for k in ("n", "F", "G", "flags")}
        rec["x"], rec["g"], rec["node_ptr"] = f32_at(a["x"], n * F), f32_at(a["g"], G * F), i64_at(a["node_ptr"], G + 1)
        if jsd:
            rec["neg"] = f32_at(a["neg"], n * F) if a["neg"] else None
        if back:
            rec["gup"] = f64_at(a["gup"], 1)
        self.calls.append((name, rec))
        if status:
            return status
        if back:
            fills = [("gh", 3.0, n * F)] + ([("gg", 5.0, G * F)] if jsd else []) + ([("gneg", 4.0, n * F)] if jsd and a["gneg"] else [])
            for key, v, count in fills:
                out = ctypes.cast(a[key], ctypes.POINTER(ctypes.c_float))
                for i in range(count):
                    out[i] = v
        else:
            ctypes.cast(a["loss"], ctypes.POINTER(ctypes.c_double))[0] = 1.5
            assert a["rows"] == a["loss"] + 8                     # one buffer: loss | rows
            out = ctypes.cast(a["rows"], ctypes.POINTER(ctypes.c_double))
            for i in range(2 * n if jsd else n):
                out[i] = -1.0
        info = a["info"]._obj
        info.rows, info.graphs, info.features, info.parts, info.arena_bytes, info.host_syncs = n, G, F, 7, ARENA, 0
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, G2lStub())


def feats(n, f, shift=0.0):
    return (torch.arange(n * f, dtype=torch.float32).reshape(n, f) / 4.0 - 1.0 + shift)


def test_arguments_of_the_jsd_exports_with_several_graphs(lib):
    h, g = feats(5, 3).requires_grad_(True), feats(2, 3, 0.5).requires_grad_(True)
    loss, rows = ops.g2l_jsd(h, g, node_ptr=[0, 2, 5], return_rows=True)
    (name, c), = lib.exports()
    assert name == "rlap_g2l_jsd" and (c["n"], c["F"], c["G"], c["flags"]) == (5, 3, 2, 0)
    assert c["x"] == h.detach().reshape(-1).tolist() and c["g"] == g.detach().reshape(-1).tolist() and c["neg"] is None
    assert c["node_ptr"] == [0, 2, 5]
    assert loss.dim() == 0 and loss.dtype == torch.float64 and float(loss.detach()) == 1.5
    assert rows.shape == (2, 5) and rows.dtype == torch.float64 and bool((rows == -1).all()) and not rows.requires_grad
    assert ops.last_stats == {"rows": 5, "graphs": 2, "features": 3, "parts": 7, "arena_bytes": ARENA, "host_syncs": 0}
    (2.5 * loss).backward()
    (_, f), (bname, b) = lib.exports()
    assert bname == "rlap_g2l_jsd_backward" and (b["n"], b["F"], b["G"], b["flags"]) == (5, 3, 2, 0)
    assert b["x"] == f["x"] and b["g"] == f["g"] and b["neg"] is None and b["node_ptr"] == [0, 2, 5] and b["gup"] == [2.5]
    assert h.grad.shape == h.shape and bool((h.grad == 3).all()) and g.grad.shape == g.shape and bool((g.grad == 5).all())


def test_arguments_of_the_jsd_exports_with_one_graph(lib):
    h, g, neg = feats(4, 3), feats(1, 3, 0.5), feats(4, 3, 9.0).requires_grad_(True)
    loss = ops.g2l_jsd(h, g, neg=neg)
    loss.backward()
    (fname, f), (bname, b) = lib.exports()
    assert (fname, bname) == ("rlap_g2l_jsd", "rlap_g2l_jsd_backward")
    assert f["node_ptr"] == [0, 4] == b["node_ptr"] and f["G"] == 1
    assert f["neg"] == neg.detach().reshape(-1).tolist() == b["neg"] and b["gup"] == [1.0]
    assert bool((neg.grad == 4).all()) and h.grad is None and g.grad is None


def test_arguments_of_the_bootstrap_exports(lib):
    h, g = feats(5, 3).requires_grad_(True), feats(2, 3, 0.5)
    table = ops.GraphTable([0, 5, 5], 5)
    loss, rows = ops.g2l_bootstrap(h, g, node_ptr=table, return_rows=True)
    assert rows.shape == (5,) and rows.dtype == torch.float64 and not rows.requires_grad and float(loss.detach()) == 1.5
    (0.5 * loss).backward()
    (fname, f), (bname, b) = lib.exports()
    assert (fname, bname) == ("rlap_g2l_bootstrap", "rlap_g2l_bootstrap_backward")
    for c in (f, b):
        assert (c["n"], c["F"], c["G"], c["flags"]) == (5, 3, 2, 0) and c["node_ptr"] == [0, 5, 5]
        assert c["x"] == h.detach().reshape(-1).tolist() and c["g"] == g.reshape(-1).tolist()
    assert b["gup"] == [0.5] and bool((h.grad == 3).all())
    assert ops.last_stats["graphs"] == 2 and ops.last_stats["host_syncs"] == 0


def test_no_graph_is_recorded_without_requires_grad(lib):
    assert not ops.g2l_jsd(feats(4, 3), feats(1, 3), neg=feats(4, 3)).requires_grad
    assert not ops.g2l_bootstrap(feats(4, 3), feats(1, 3)).requires_grad
    h = feats(4, 3).requires_grad_(True)
    with torch.no_grad():
        assert not ops.g2l_bootstrap(h, feats(1, 3)).requires_grad
    assert [c[0] for c in lib.exports()] == ["rlap_g2l_jsd", "rlap_g2l_bootstrap", "rlap_g2l_bootstrap"]


def test_non_contiguous_inputs_are_packed(lib):
    h = feats(3, 5).t()          # (5, 3), strided
    ops.g2l_bootstrap(h, feats(1, 3))
    (_, c), = lib.exports()
    assert c["x"] == h.contiguous().reshape(-1).tolist() and (c["n"], c["F"]) == (5, 3)


Z = torch.zeros
JSD_BAD = [
    dict(h=Z(5), g=Z(1, 3), neg=Z(5)),                                          # not 2-D
    dict(h=Z(1, 5, 3), g=Z(1, 3), neg=Z(1, 5, 3)),
    dict(h=Z(5, 3), g=Z(3), neg=Z(5, 3)),
    dict(h=Z(5, 3, dtype=torch.float64), g=Z(1, 3, dtype=torch.float64), neg=Z(5, 3, dtype=torch.float64)),   # not float32
    dict(h=Z(5, 3), g=Z(1, 3, dtype=torch.float16), neg=Z(5, 3)),
    dict(h=Z(5, 3), g=Z(1, 3), neg=Z(5, 3, dtype=torch.float64)),
    dict(h=[[1.0, 2.0]], g=Z(1, 2), neg=Z(1, 2)),                               # not a tensor
    dict(h=Z(0, 3), g=Z(1, 3), neg=Z(0, 3)),                                    # no row
    dict(h=Z(5, 0), g=Z(1, 0), neg=Z(5, 0)),                                    # no column
    dict(h=Z(5, 3), g=Z(0, 3), node_ptr=[0]),                                   # no graph
    dict(h=Z(5, 3), g=Z(1, 4), neg=Z(5, 3)),                                    # F differs
    dict(h=Z(2, 513), g=Z(1, 513), neg=Z(2, 513)),                              # F > 512
    dict(h=Z(5, 3), g=Z(1, 3), neg=Z(4, 3)),                                    # neg's shape
    dict(h=Z(5, 3), g=Z(1, 3)),                                                 # one graph without neg
    dict(h=Z(5, 3), g=Z(1, 3), node_ptr=[0, 5]),
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[0, 2, 5], neg=Z(5, 3)),                # several graphs with neg
    dict(h=Z(5, 3), g=Z(2, 3)),                                                 # several graphs without a table
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[0, 5]),                                # the table's graphs are not g's
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[0, 2, 4]),                             # the table does not end at N
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[0, 6, 5]),                             # decreasing
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[1, 2, 5]),                             # does not start at 0
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=ops.GraphTable([0, 2, 6], 6)),          # a table of another batch
]
BOOT_BAD = [
    dict(h=Z(5), g=Z(1, 3)),                                                    # not 2-D
    dict(h=Z(5, 3), g=Z(3)),
    dict(h=Z(5, 3, dtype=torch.float64), g=Z(1, 3, dtype=torch.float64)),       # not float32
    dict(h=Z(5, 3), g=Z(1, 3, dtype=torch.float16)),
    dict(h=[[1.0, 2.0]], g=Z(1, 2)),                                            # not a tensor
    dict(h=Z(0, 3), g=Z(1, 3)),                                                 # no row
    dict(h=Z(5, 0), g=Z(1, 0)),                                                 # no column
    dict(h=Z(5, 3), g=Z(0, 3), node_ptr=[0]),                                   # no graph
    dict(h=Z(5, 3), g=Z(1, 4)),                                                 # F differs
    dict(h=Z(2, 513), g=Z(1, 513)),                                             # F > 512
    dict(h=Z(5, 3), g=Z(2, 3)),                                                 # several graphs without a table
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[0, 5]),                                # the table's graphs are not g's
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[0, 2, 4]),                             # the table does not end at N
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[0, 6, 5]),                             # decreasing
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=[1, 2, 5]),                             # does not start at 0
    dict(h=Z(5, 3), g=Z(2, 3), node_ptr=ops.GraphTable([0, 2, 6], 6)),          # a table of another batch
    dict(h=Z(5, 3), g=Z(1, 3).requires_grad_(True)),                            # the targets are constants
]


def _reached(*args, **kw):
    raise AssertionError("the device or the library was reached")


@pytest.mark.parametrize("kw", JSD_BAD)
def test_bad_jsd_arguments_raise_value_error_before_any_call(lib, monkeypatch, kw):
    monkeypatch.setattr(ops, "_device_for", _reached)
    monkeypatch.setattr(ops, "_handle_obj", _reached)
    with pytest.raises(ValueError):
        ops.g2l_jsd(**kw)
    assert lib.exports() == []


@pytest.mark.parametrize("kw", BOOT_BAD)
def test_bad_bootstrap_arguments_raise_value_error_before_any_call(lib, monkeypatch, kw):
    monkeypatch.setattr(ops, "_device_for", _reached)
    monkeypatch.setattr(ops, "_handle_obj", _reached)
    with pytest.raises(ValueError):
        ops.g2l_bootstrap(**kw)
    assert lib.exports() == []


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (7, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    before = ops.last_stats
    with pytest.raises(exc, match=f"status {status}"):
        ops.g2l_bootstrap(feats(4, 2), feats(1, 2))
    with pytest.raises(exc, match=f"status {status}"):
        ops.g2l_jsd(feats(4, 2), feats(1, 2), neg=feats(4, 2))
    assert ops.last_stats is before


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.g2l_jsd(feats(4, 2), feats(2, 2), node_ptr=[0, 1, 4])
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_g2l_jsd")
    assert names[i:i + 4] == ["rlap_g2l_jsd", "rlap_workspace_needed", "rlap_set_workspace", "rlap_g2l_jsd"]
    assert lib.calls[i + 2][1]["ws_bytes"] >= 1 << 20


def test_g2l_info_layout(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_g2l_info", "G2lInfo")
    assert [f for f, _ in _lib.G2lInfo._fields_] == ["rows", "graphs", "features", "parts", "arena_bytes", "host_syncs", "pad"]
    assert ctypes.sizeof(_lib.G2lInfo) % 8 == 0


def test_exports_are_declared():
    assert set(SIGS) <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    block = hdr[hdr.index("The fused graph-to-local losses"):hdr.index("} rlap_g2l_info;")]
    assert "not finite" in block and "never an access out of range" in block


# ------------------------------------------------------------------------------------------------ the adapters
def test_g2l_contrast_with_one_graph(lib):
    h1, h2 = feats(4, 3).requires_grad_(True), feats(4, 3, 0.5).requires_grad_(True)
    g1, g2 = feats(1, 3, 2.0).requires_grad_(True), feats(1, 3, 3.0).requires_grad_(True)
    h3, h4 = feats(4, 3, 5.0), feats(4, 3, 6.0)
    loss = adapters.G2LContrast()(h1, h2, g1, g2, h3, h4)
    assert float(loss.detach()) == 1.5 and loss.dtype == torch.float64            # 0.5 * (1.5 + 1.5)
    x, y = lib.exports()
    assert x[0] == y[0] == "rlap_g2l_jsd"
    flat = lambda t: t.detach().reshape(-1).tolist()
    assert (x[1]["x"], x[1]["g"], x[1]["neg"]) == (flat(h2), flat(g1), flat(h4))
    assert (y[1]["x"], y[1]["g"], y[1]["neg"]) == (flat(h1), flat(g2), flat(h3))
    loss.backward()
    back = [c for c in lib.exports() if c[0] == "rlap_g2l_jsd_backward"]
    assert len(back) == 2 and sorted(c[1]["gup"] for c in back) == [[0.5], [0.5]]
    assert bool((h1.grad == 3).all()) and bool((g2.grad == 5).all())
    with pytest.raises(ValueError):
        adapters.G2LContrast()(h1, h2, g1, g2)                                    # one graph needs the corrupted pass


def test_g2l_contrast_with_several_graphs_and_stacked_views(lib):
    h = torch.stack([feats(5, 3), feats(5, 3, 0.5), feats(5, 3, 9.0)])
    g = torch.stack([feats(2, 3, 1.0), feats(2, 3, 2.0)])
    adapters.G2LContrast()(h, g1=g, node_ptr=[0, 2, 5])
    x, y = lib.exports()
    flat = lambda t: t.reshape(-1).tolist()
    assert (x[1]["x"], x[1]["g"], x[1]["neg"], x[1]["node_ptr"]) == (flat(h[1]), flat(g[0]), None, [0, 2, 5])
    assert (y[1]["x"], y[1]["g"]) == (flat(h[0]), flat(g[1]))
    with pytest.raises(ValueError):
        adapters.G2LContrast()(h[0], h[1], g[0], g[1], feats(5, 3), feats(5, 3), node_ptr=[0, 2, 5])   # several graphs take no h3 / h4
    with pytest.raises(ValueError):
        adapters.G2LContrast()(h[:1], g1=g, node_ptr=[0, 2, 5])


def test_bootstrap_g2l_detaches_the_targets(lib):
    h1, h2 = feats(5, 3).requires_grad_(True), feats(5, 3, 0.5).requires_grad_(True)
    g1, g2 = feats(2, 3, 1.0).requires_grad_(True), feats(2, 3, 2.0).requires_grad_(True)
    loss = adapters.BootstrapG2L()(h1, h2, g1, g2, node_ptr=[0, 2, 5])
    x, y = lib.exports()
    flat = lambda t: t.detach().reshape(-1).tolist()
    assert x[0] == y[0] == "rlap_g2l_bootstrap"
    assert (x[1]["x"], x[1]["g"]) == (flat(h2), flat(g1)) and (y[1]["x"], y[1]["g"]) == (flat(h1), flat(g2))
    loss.backward()
    assert bool((h1.grad == 3).all()) and bool((h2.grad == 3).all()) and g1.grad is None and g2.grad is None
    stacked = adapters.BootstrapG2L()(torch.stack([h1, h2]).detach(), g1_target=torch.stack([g1, g2]).detach(), node_ptr=[0, 2, 5])
    assert float(stacked) == 1.5


def test_corrupt_is_a_row_permutation():
    x = feats(50, 3)
    gen = torch.Generator().manual_seed(4)
    y = adapters.corrupt(x, generator=gen)
    assert y.shape == x.shape and not torch.equal(x, y)
    assert torch.equal(torch.sort(y[:, 0]).values, x[:, 0])
    assert torch.equal(y, x[torch.randperm(50, generator=torch.Generator().manual_seed(4))])
