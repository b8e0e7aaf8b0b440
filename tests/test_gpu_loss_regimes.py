"""The three fused loss families on the device -- InfoNCE (rlap_infonce.hip), CCA-SSG (rlap_cca.hip, 4.16), the graph-to-
local JSD and bootstrap losses (rlap_g2l.hip, 4.17) -- regime by regime: what their launchers can choose (infonce::main_instance,
cca::gram_instance, cca::zr_instance, g2l::vec_rows and the three num_parts) and what tests/test_gpu_infonce.py, test_gpu_cca.py and
test_gpu_g2l.py do not reach.  The mirrors, their caches, the input generators and the helpers are those files'; so is every rule
of comparison, and there is no new tolerance:

  bit for bit   InfoNCE Z, ga, gb; CCA colstat, gram, terms, dh1, dh2; JSD dh, dneg, dg; bootstrap c_i, dh and the loss;
  1e-13         what passes a device log or log1p: InfoNCE's rows (the neighbour rule of test_gpu_infonce.py, then 1e-13 absolute)
                and loss; JSD's loss, pos_i and neg_i (REL = 1e-13 relative to the mirror's value, element by element).

  a. the feature sweep: N = 161 (six row tiles in two row blocks, the second with two live waves, the last tile with one live row,
     an odd N for CCA's row pair) and, for every count t = 1 .. 16 of 32-column tiles, F = 32 (t - 1) + 1 (one live column in the
     last tile) and F = 32 t: every template instance at every fill, dead accumulator tiles and dead prefetch registers included;
     the Gram product's odd tile counts (a clamped tile computed twice, stored once), 1 to 9 pair groups, a last group of one, two
     and three live waves; waves of the zr kernel that own different numbers of column tiles.  Five calls per F, forward and
     backward with the upstream gradient 0.75: InfoNCE, CCA, JSD with 33 graphs, JSD with one graph, the bootstrap with 33 graphs.
  b. the vector kernels on both sides of every edge of g2l::vec_rows (F = 65 | 66, 131 | 132, 263 | 264: 256, 128, 64, 32 rows a
     block) at N = 513: 3, 5, 9, 17 blocks, the last with one row.
  c. parts set by the target and not by the tile count: JSD and bootstrap with 129 graphs over 4129 nodes (128 parts over 130 tiles,
     uneven parts, two row blocks of graphs, the second with one live wave); one graph over 32,801 nodes (the cap of 1024 parts over
     1026 tiles); CCA at (1000, 500) (29 parts over 32 tiles, nine pair groups, a last column tile partly filled); InfoNCE at
     N = 1024 (32 parts = T) and 1056 (29 parts < T = 33).
  d. InfoNCE in the single-part regime, N = 32,641 (the regime of the workloads of 34,493 and 169,343 rows), with the exact data of
     test_operand_maps_with_exact_data: every similarity depends on the anchor only through its class i mod F, so Z is a count per
     class (bit for bit) and the gradients have a float64 statement by class of O(N F) work (by_class below), held to GRAD_BOUND of
     tests/test_infonce_cpu.py relative to the largest entry.  The same structure gives the rule's own bits in O(N^2 / F)
     (rule_by_class), which ga and gb equal bit for bit.  tests/test_loss_regimes_cpu.py holds both against the mirror and the
     statement against autograd at N = 2708.
  e. one partially filled case per family again with a poisoned arena: equal bits, so a dead accumulator tile or a pad column that
     leaks is seen.

tests/test_loss_regimes_cpu.py feeds the case lists below through the exported rules and asserts that every regime is reached.
Every comparison within 1e-13 prints its figure before it asserts.
"""
import numpy as np
import pytest
import torch

import infonce_mirror as im
import test_gpu_cca as tc
import test_gpu_g2l as tg
import test_gpu_infonce as ti
from test_gpu_cca import mirror as mirror_cca  # noqa: F401  (fixtures: the mirrors of the three files, each with its cache)
from test_gpu_g2l import mirror as mirror_g2l  # noqa: F401
from test_gpu_infonce import mirror as mirror_in, ops  # noqa: F401
from test_infonce_cpu import GRAD_BOUND

pytestmark = pytest.mark.gpu

G_UP = 0.75
assert ti.G_UP == tc.G_UP == tg.G_UP == G_UP           # the mirrors' caches hold the gradients of this upstream value

# ---- the case lists (tests/test_loss_regimes_cpu.py reads them)
SWEEP_N = 161
SWEEP_F = [f for t in range(1, 17) for f in (32 * (t - 1) + 1, 32 * t)]
SWEEP_G = 33
POSITIVES, TAUS = ("scaled", "raw"), (0.4, 1.0 / 32.0, 2.0)
INFONCE_SWEEP = [(SWEEP_N, f, POSITIVES[k % 2], TAUS[k % 3]) for k, f in enumerate(SWEEP_F)]
CCA_SWEEP = [(SWEEP_N, f, tc.LAMBDS[k % 3]) for k, f in enumerate(SWEEP_F)]
JSD_MANY_SWEEP = [(SWEEP_N, SWEEP_G, f, "empty") for f in SWEEP_F]
JSD_ONE_SWEEP = [(SWEEP_N, 1, f, None) for f in SWEEP_F]
BOOT_SWEEP = [(SWEEP_N, SWEEP_G, f, "empty") for f in SWEEP_F]

VEC_N, VEC_G = 513, 5
VEC_F = [65, 66, 131, 132, 263, 264]
JSD_ONE_VEC = [(VEC_N, 1, f, None) for f in VEC_F]
BOOT_VEC = [(VEC_N, VEC_G, f, "even") for f in VEC_F]

JSD_MANY_PARTS = [(4129, 129, 33, "even")]
BOOT_PARTS = [(4129, 129, 33, "even")]
JSD_ONE_PARTS = [(32801, 1, 3, None)]
CCA_PARTS = [(1000, 500, tc.LAMBDS[0])]
INFONCE_PARTS = [(1024, 3, "raw", 0.4), (1056, 3, "scaled", 2.0)]

SINGLE_PART = (32641, 8, "raw", 2.0)                    # (N, F, positive, tau)

POISON_INFONCE = (SWEEP_N, 65, "raw", 0.4)
POISON_CCA = (SWEEP_N, 161, tc.LAMBDS[0])
POISON_JSD = (SWEEP_N, SWEEP_G, 65, "empty")

INFONCE_CASES = INFONCE_SWEEP + INFONCE_PARTS
CCA_CASES = CCA_SWEEP + CCA_PARTS
JSD_MANY_CASES = JSD_MANY_SWEEP + JSD_MANY_PARTS
JSD_ONE_CASES = JSD_ONE_SWEEP + JSD_ONE_VEC + JSD_ONE_PARTS
BOOT_CASES = BOOT_SWEEP + BOOT_VEC + BOOT_PARTS


def gup(t):
    return torch.tensor(G_UP, dtype=torch.float64, device=t.device)


# ------------------------------------------------------------------------------------------------ one call of each family
def infonce_call(ops, a, b, positive, tau):
    """Forward and backward on the device: Z, the loss, the rows, ga, gb."""
    ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    z = ti.forward_z(ops, ta.detach(), tb.detach(), tau, positive)
    loss, rows = ops.info_nce(ta, tb, tau=tau, positive=positive, return_rows=True)
    st = dict(ops.last_stats)
    loss.backward(gup(loss))
    assert ops.last_stats["host_syncs"] == 0 and st["host_syncs"] == 0 and (st["rows"], st["features"]) == a.shape
    return {"z": z, "loss": loss.detach(), "rows": rows, "ga": ta.grad, "gb": tb.grad, "parts": st["parts"]}


def infonce_case(ops, mirror, n, f, positive, tau):
    a, b = ti.views(n, f)
    m = mirror(n, f, positive, tau)
    out = infonce_call(ops, a, b, positive, tau)
    assert out["parts"] == mirror.lib.infonce_parts(n)
    assert ti.bits(out["z"]) == ti.bits(m["z"]), "Z" + ti.where(out["z"].cpu().numpy(), m["z"])
    err = ti.rows_against_the_mirror(out["rows"], m, positive, tau)
    print(f"infonce n={n} F={f} {positive} tau={tau}: rows max |diff| {err:.3g}, loss diff {abs(float(out['loss']) - m['loss']):.3g}")
    assert err <= 1e-13
    assert abs(float(out["loss"]) - m["loss"]) <= 1e-13
    assert ti.bits(out["ga"]) == ti.bits(m["ga"]), "ga" + ti.where(out["ga"].cpu().numpy(), m["ga"])
    assert ti.bits(out["gb"]) == ti.bits(m["gb"]), "gb" + ti.where(out["gb"].cpu().numpy(), m["gb"])
    return out


def cca_call(ops, a, b, lambd):
    ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    terms, colstat, gram, _, _ = ops._cca_forward(ta.detach(), tb.detach(), float(lambd))
    st = dict(ops.last_stats)
    loss = ops.cca_loss(ta, tb, lambd=lambd)
    loss.backward(gup(loss))
    assert ops.last_stats["host_syncs"] == 0 and st["host_syncs"] == 0 and (st["rows"], st["features"]) == a.shape
    return {"terms": terms, "colstat": colstat, "gram": gram, "loss": loss.detach(), "ga": ta.grad, "gb": tb.grad, "parts": st["parts"]}


def cca_case(ops, mirror, n, f, lambd):
    a, b = tc.views(n, f)
    m = mirror(n, f, lambd)
    out = cca_call(ops, a, b, lambd)
    assert out["parts"] == mirror.lib.cca_parts(n, f)
    tc.same("colstat", out["colstat"], m["colstat"])
    tc.same("gram", out["gram"], m["gram"])
    tc.same("terms", out["terms"], m["terms"])
    tc.same("cca_loss", out["loss"], m["terms"][0])
    tc.same("dh1", out["ga"], m["ga"])
    tc.same("dh2", out["gb"], m["gb"])
    return out


def jsd_call(ops, h, g, neg, t):
    th, tgr = tg.cuda(h).requires_grad_(True), tg.cuda(g).requires_grad_(True)
    tn = tg.cuda(neg).requires_grad_(True) if neg is not None else None
    loss, rows = ops.g2l_jsd(th, tgr, node_ptr=t, neg=tn, return_rows=True)
    st = dict(ops.last_stats)
    loss.backward(gup(loss))
    assert ops.last_stats["host_syncs"] == 0 and st["host_syncs"] == 0
    assert (st["rows"], st["graphs"], st["features"]) == (h.shape[0], g.shape[0], h.shape[1])
    return {"loss": loss.detach(), "rows": rows, "gh": th.grad, "gg": tgr.grad, "gneg": tn.grad if tn is not None else None, "parts": st["parts"]}


def jsd_case(ops, mirror, n, G, f, kind):
    h, g, neg = tg.inputs(n, G, f)
    m = mirror("jsd", n, G, f, kind)
    out = jsd_call(ops, h, g, neg, tg.table_of(n, G, kind))
    assert out["parts"] == mirror.lib.g2l_parts(n, G, f)
    rows = out["rows"].cpu().numpy()
    el, ep, en = tg.close(float(out["loss"]), m["loss"]), tg.close(rows[0], m["pos"]), tg.close(rows[1], m["neg"])
    print(f"jsd n={n} G={G} F={f}: loss rel {el:.3g}, pos rel {ep:.3g}, neg rel {en:.3g}; largest |diff| pos {np.abs(rows[0] - m['pos']).max():.3g}, "
          f"neg {np.abs(rows[1] - m['neg']).max():.3g}")
    assert el <= tg.REL and ep <= tg.REL and en <= tg.REL
    tg.same(out["gh"], m["gh"], "dh")
    tg.same(out["gg"], m["gg"], "dg")
    if neg is not None:
        tg.same(out["gneg"], m["gneg"], "dneg")
    return out


def boot_call(ops, h, g, t):
    th = tg.cuda(h).requires_grad_(True)
    loss, rows = ops.g2l_bootstrap(th, tg.cuda(g), node_ptr=t, return_rows=True)
    st = dict(ops.last_stats)
    loss.backward(gup(loss))
    assert ops.last_stats["host_syncs"] == 0 and (st["rows"], st["graphs"], st["features"], st["host_syncs"]) == (h.shape[0], g.shape[0], h.shape[1], 0)
    return {"loss": loss.detach(), "rows": rows, "gh": th.grad}


def boot_case(ops, mirror, n, G, f, kind):
    h, g, _ = tg.inputs(n, G, f)
    m = mirror("bootstrap", n, G, f, kind)
    out = boot_call(ops, h, g, tg.table_of(n, G, kind))
    tg.same(out["rows"], m["c"], "c")
    assert tg.bits(out["loss"]) == tg.bits(np.float64(m["loss"])), (float(out["loss"]), m["loss"])
    tg.same(out["gh"], m["gh"], "dh")
    return out


def ids(cases):
    return ["-".join(str(round(x, 4) if isinstance(x, float) else x) for x in c) for c in cases]


# ------------------------------------------------------------------------------------------------ a, b, c: against the mirrors
@pytest.mark.parametrize("n,f,positive,tau", INFONCE_CASES, ids=ids(INFONCE_CASES))
def test_infonce(ops, mirror_in, n, f, positive, tau):
    infonce_case(ops, mirror_in, n, f, positive, tau)


@pytest.mark.parametrize("n,f,lambd", CCA_CASES, ids=ids(CCA_CASES))
def test_cca(ops, mirror_cca, n, f, lambd):
    cca_case(ops, mirror_cca, n, f, lambd)


@pytest.mark.parametrize("n,G,f,kind", JSD_MANY_CASES, ids=ids(JSD_MANY_CASES))
def test_jsd_many_graphs(ops, mirror_g2l, n, G, f, kind):
    jsd_case(ops, mirror_g2l, n, G, f, kind)


@pytest.mark.parametrize("n,G,f,kind", JSD_ONE_CASES, ids=ids(JSD_ONE_CASES))
def test_jsd_one_graph(ops, mirror_g2l, n, G, f, kind):
    jsd_case(ops, mirror_g2l, n, G, f, kind)


@pytest.mark.parametrize("n,G,f,kind", BOOT_CASES, ids=ids(BOOT_CASES))
def test_bootstrap(ops, mirror_g2l, n, G, f, kind):
    boot_case(ops, mirror_g2l, n, G, f, kind)


# ------------------------------------------------------------------------------------------------ d: InfoNCE, one part
def by_class(lib, b, tau, positive, g):
    """The InfoNCE loss on ti.exact_views(n, f) stated by class, in O(N F): a_i = e_(i mod F) has norm 1 and b_j norm 2, so ah = a,
    bh = b / 2 and s_ij = bh_j[i mod F] exactly -- 0 or +-0.5, the same for every anchor i of a class.
      z, rows   the float64 values the rule gives: Z of a class is a count of three expw values (multiples of 2^-25 with a sum below
                2^15: the float64 sum is exact in any order);
      ga, gb    float64 mathematics, no rule: with P_cj = exp(s_cj / tau) / sum_j exp(s_cj / tau),
                d loss / d ah_i = -(g / N) (c bh_i - (1 / tau) sum_j P_(class i),j bh_j),
                d loss / d bh_j = -(g / N) (c ah_j - (1 / tau) sum_i P_(class i),j ah_i), the inner sum being count_k P_kj in column k,
                both pushed through the normalisation x -> x / |x|."""
    n, f = b.shape
    cls = np.arange(n) % f
    bh = b.astype(np.float64) / 2.0
    S = bh.T.copy()                                                            # S[c, j] = s_ij of every i of class c
    assert np.isin(S, (-0.5, 0.0, 0.5)).all()
    itf = np.float32(1.0 / tau)
    e = {v: np.float64(im.expw(lib, np.array([(np.float32(v) - np.float32(1.0)) * itf], dtype=np.float32))[0]) for v in (-0.5, 0.0, 0.5)}
    z = sum((S == v).sum(axis=1) * e[v] for v in (-0.5, 0.0, 0.5))[cls]
    c = 1.0 if positive == "raw" else 1.0 / tau
    rows = c * S[cls, np.arange(n)] - 1.0 / tau - np.log(z)
    P = np.exp(S / tau)
    P /= P.sum(axis=1, keepdims=True)
    ah = np.zeros((n, f))
    ah[np.arange(n), cls] = 1.0
    gs = -(g / n)
    Ga = gs * (c * bh - (P @ bh)[cls] / tau)
    Gb = gs * (c * ah - (np.bincount(cls, minlength=f)[:, None] * P).T / tau)
    ga = (Ga - ah * (ah * Ga).sum(axis=1, keepdims=True)) / 1.0
    gb = (Gb - bh * (bh * Gb).sum(axis=1, keepdims=True)) / 2.0
    return {"z": z, "rows": rows, "loss": -rows.mean(), "ga": ga, "gb": gb}


def rule_by_class(lib, b, tau, positive, g):
    """ga, gb of rlap_infonce.h's rule on the same data, bit for bit, in O(N^2 / F) vectorised work: what the mirror would give
    had it the time.  p_ij = e(s_(class i),j) * (float)(1 / Z_(class i)) takes one value per (class, j), and every product of the
    chains is exact (bh is 0 or +-0.5, ah is 0 or 1), so a step fmaf(p, x, acc) is the float32 sum acc + p x, or acc where x = 0:
      D    of an anchor depends on its class alone: F chains over the samples in the header's order (parts, tiles, registers,
           halves), F columns each;
      D'   of sample j in column k adds P_kj once per anchor of class k in the part, whatever their order;
    then the float64 push through the normalisation with the header's operations in their order (norms 1 and 2, never clamped)."""
    n, f = b.shape
    cls = np.arange(n) % f
    bh = (b / np.float32(2.0)).astype(np.float32)
    S = bh.T.copy()
    itf = np.float32(1.0 / tau)
    e32 = np.zeros((f, n), dtype=np.float32)
    for v in (-0.5, 0.0, 0.5):
        e32[S == np.float32(v)] = im.expw(lib, np.array([(np.float32(v) - np.float32(1.0)) * itf], dtype=np.float32))[0]
    zc = e32.astype(np.float64).sum(axis=1)                                     # exact in any order
    P = e32 * (1.0 / zc).astype(np.float32)[:, None]                           # (F, N) float32: prob(e, recip_z(Z))
    parts = lib.infonce_parts(n)
    begin = [lib.infonce_part_begin(n, p) for p in range(parts + 1)]
    order = [lib.infonce_reg_row(r, h) for r in range(16) for h in range(2)]
    D = np.zeros((f, f), dtype=np.float32)                                      # [class, column]
    Dp = np.zeros((n, f), dtype=np.float32)
    PT = np.ascontiguousarray(P.T)                                              # [j, k]
    for p in range(parts):
        acc = np.zeros((f, f), dtype=np.float32)
        for t in range(begin[p], begin[p + 1]):
            for o in order:
                j = 32 * t + o
                if j < n:
                    acc = acc + P[:, j, None] * bh[None, j, :]
        D = D + acc
        lo, hi = 32 * begin[p], min(n, 32 * begin[p + 1])
        count = np.bincount(cls[lo:hi], minlength=f)                            # the part's anchors of each class
        accp = np.zeros((n, f), dtype=np.float32)
        for step in range(count.min()):
            accp += PT
        for step in range(count.min(), count.max()):
            accp = np.where((step < count)[None, :], accp + PT, accp)
        Dp = Dp + accp
    assert D.dtype == np.float32 and Dp.dtype == np.float32
    ah = np.zeros((n, f), dtype=np.float32)
    ah[np.arange(n), cls] = 1.0
    c, itau, gs = (1.0 if positive == "raw" else 1.0 / tau), 1.0 / tau, -(g / float(n))

    def push(own, other, chain, nrm):
        G = gs * (c * other.astype(np.float64) - itau * chain.astype(np.float64))
        dot = np.zeros(n)
        for k in range(f):
            dot = dot + own[:, k].astype(np.float64) * G[:, k]
        return ((G - own.astype(np.float64) * dot[:, None]) / nrm).astype(np.float32)
    return {"ga": push(ah, bh, D[cls], 1.0), "gb": push(bh, ah, Dp, 2.0)}


def grad_rel(ga, gb, want):
    """The largest difference of either gradient, relative to the largest entry of both (as tests/test_infonce_cpu.py)."""
    gmax = max(np.abs(want["ga"]).max(), np.abs(want["gb"]).max())
    return max(np.abs(ga - want["ga"]).max(), np.abs(gb - want["gb"]).max()) / gmax


def test_infonce_single_part(ops, mirror_in):
    n, f, positive, tau = SINGLE_PART
    assert mirror_in.lib.infonce_parts(n) == 1 and mirror_in.lib.infonce_parts(n - 1) == 2     # the first N of the regime
    a, b = ti.exact_views(n, f)
    want = by_class(mirror_in.lib, b, tau, positive, G_UP)
    out = infonce_call(ops, a, b, positive, tau)
    assert out["parts"] == 1
    z = out["z"].cpu().numpy()
    assert ti.bits(z) == ti.bits(want["z"]), "Z" + ti.where(z, want["z"])
    err = np.abs(out["rows"].cpu().numpy() - want["rows"]).max()
    rel = grad_rel(out["ga"].cpu().numpy().astype(np.float64), out["gb"].cpu().numpy().astype(np.float64), want)
    print(f"infonce n={n} F={f} {positive} tau={tau}, one part: rows max |diff| {err:.3g}, loss diff {abs(float(out['loss']) - want['loss']):.3g}, "
          f"gradients rel {rel:.3g} (bound {GRAD_BOUND:.3g})")
    assert err <= 1e-13                                                        # s_ii exact: the class's entry, not a neighbour's
    assert rel <= GRAD_BOUND
    assert bool(torch.isfinite(out["ga"]).all()) and bool(torch.isfinite(out["gb"]).all())
    # and the rule's own bits: on this data a chain of 32,641 float32 steps adds three values again and again, so its rounding is
    # systematic and takes up most of the bound (the rule against the statement is printed too); the device must add none of its own
    rule = rule_by_class(mirror_in.lib, b, tau, positive, G_UP)
    print(f"  the rule against the float64 statement: gradients rel {grad_rel(rule['ga'].astype(np.float64), rule['gb'].astype(np.float64), want):.3g}")
    assert ti.bits(out["ga"]) == ti.bits(rule["ga"]), "ga" + ti.where(out["ga"].cpu().numpy(), rule["ga"])
    assert ti.bits(out["gb"]) == ti.bits(rule["gb"]), "gb" + ti.where(out["gb"].cpu().numpy(), rule["gb"])


# ------------------------------------------------------------------------------------------------ e: a poisoned arena
def all_bits(out):
    return {k: ti.bits(v) for k, v in out.items() if isinstance(v, torch.Tensor)}


def poisoned(ops, call):
    base = all_bits(call())
    ops.debug_set_poison(0xFF)
    try:
        again = all_bits(call())
    finally:
        ops.debug_set_poison(-1)
    assert sorted(again) == sorted(base)
    for key in base:
        assert again[key] == base[key], f"{key} depends on what the arena held"


def test_infonce_partially_filled_with_a_poisoned_arena(ops, mirror_in):
    poisoned(ops, lambda: infonce_case(ops, mirror_in, *POISON_INFONCE))


def test_cca_partially_filled_with_a_poisoned_arena(ops, mirror_cca):
    poisoned(ops, lambda: cca_case(ops, mirror_cca, *POISON_CCA))


def test_g2l_partially_filled_with_a_poisoned_arena(ops, mirror_g2l):
    poisoned(ops, lambda: jsd_case(ops, mirror_g2l, *POISON_JSD))
    poisoned(ops, lambda: boot_case(ops, mirror_g2l, *POISON_JSD))
