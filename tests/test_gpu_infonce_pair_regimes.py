"""The symmetric InfoNCE pair on the device (ops.info_nce_pair, rlap_infonce_pair / rlap_infonce_pair_backward) regime by
regime: what its launchers can choose -- the five instances of k_in_main<NFT, IN_BACK_PAIR> at every fill, the backward's
infonce::num_parts, and the forward's own split (pair_groups, pair_parts, PAIR_SPAN_TILES of k_in_pair_main) -- and what
tests/test_gpu_infonce_pair.py does not reach.  The mirror, its cache, the input generators and the helpers are that file's; so is
every rule of comparison (bit for bit: Z, Zc, ga, gb; the rows by the neighbour rule and then within 1e-13; the loss within 1e-13),
and the one new measured figure is SINGLE_PART_GRAD_BOUND of tests/test_infonce_pair_regimes_cpu.py, measured on the CPU.

  a. the feature sweep: N = 161 (six row tiles in two row blocks, the second with two live waves, the last tile with one live row)
     and, for every count t = 1 .. 16 of 32-column tiles, F = 32 (t - 1) + 1 and F = 32 t: every instance of the backward ladder at
     every fill, dead accumulator tiles included.  Forward and backward with the upstream gradient 0.75.
  b. the work-split edges (SPLIT below), F = 3: the backward's parts == T and parts < T; the forward's one tile per part up to
     N = 1408, then parts of one and two tiles, the first N of 16 groups, all parts of two tiles, the first group of two row blocks.
     parts, groups and the span of every case are asserted against the table, which tests/test_infonce_pair_regimes_cpu.py holds
     against the header's formulas.
  c. the single-part backward, N = 32,641 (the regime of the workloads of 34,493 and 169,343 rows), with the exact data of
     test_operand_maps_with_exact_data: every similarity depends on the anchor only through its class i mod F, so Z is a count per
     class and Zc a count per column (bit for bit), the gradients have a float64 statement of O(N F) work (pair_by_class) and the
     rule's own bits come in O(N^2 / F) (pair_rule_by_class), which ga and gb equal bit for bit.
  d. a part of two spans, forward only, N = 262,145 (T = 8193: 31 parts of 256 tiles and one of 257, whose second span is one tile
     with one live row): the only regime in which k_in_pair_main re-reads a part sum, clears its column array a second time and
     flushes at a span's offset.  Z and Zc are counts (bit for bit), the rows within 1e-13, the loss within the worst-case bound of
     any summation order.
  e. two partially filled cases again with a poisoned arena: equal bits, so a dead accumulator tile that leaks is seen.

tests/test_infonce_pair_regimes_cpu.py feeds the case lists below through the exported rules and asserts that every regime is
reached, and holds the two host statements against the pair's mirror and autograd at N = 2708.  Every comparison within a bound
prints its figure before it asserts.
"""
import math
import time

import numpy as np
import pytest
import torch

import infonce_mirror as im
import infonce_pair_mirror as pm
from test_gpu_infonce_pair import mirror, ops  # noqa: F401  (fixtures: the pair's mirror with its cache, and the library)
from test_gpu_infonce_pair import G_UP, bits, exact_views, forward_z, rows_against_the_mirror, views, where

pytestmark = pytest.mark.gpu

# ---- the case lists (tests/test_infonce_pair_regimes_cpu.py reads them)
SWEEP_N = 161
SWEEP_F = [f for t in range(1, 17) for f in (32 * (t - 1) + 1, 32 * t)]
POSITIVES, TAUS = ("scaled", "raw"), (0.4, 1.0 / 32.0, 2.0)
SWEEP = [(SWEEP_N, f, POSITIVES[k % 2], TAUS[k % 3]) for k, f in enumerate(SWEEP_F)]

SPLIT_F = 3
#        N     forward parts, groups, span tiles      what it is the smallest / first for
SPLIT = [(1024, 32, 8, 1),                          # backward num_parts == T == 32
         (1056, 33, 9, 1),                          # backward 29 parts < T = 33; forward 9 groups x 33 parts
         (1408, 44, 11, 1),                         # the last N with one tile per forward part
         (1409, 43, 12, 2),                         # the first with pair_parts < T = 45: parts of 1 and 2 tiles; last block: one wave, one row
         (1920, 35, 15, 2),                         # 15 groups, 35 parts
         (1921, 32, 16, 2),                         # the first with 16 groups; T = 61
         (2048, 32, 16, 2),                         # all parts two tiles, all blocks full
         (2049, 32, 16, 3)]                         # the first group of two row blocks; parts of 2 and 3 tiles; last block: one wave, one row
SPLIT_CASES = [(n, SPLIT_F, POSITIVES[k % 2], TAUS[k % 3]) for k, (n, _, _, _) in enumerate(SPLIT)]
SPLIT_WANT = {n: (parts, groups, span) for n, parts, groups, span in SPLIT}

SINGLE_PART = (32641, 8, "raw", 2.0)                # (N, F, positive, tau): the shape and the data of test_infonce_single_part
TWO_SPANS = (262145, 8, "raw", 0.25)

POISON = [(SWEEP_N, 65, "raw", 0.4),                # nft 3 in instance 4: one dead tile
          (SWEEP_N, 257, "raw", 0.4)]               # nft 9 in instance 16: seven dead tiles

CASES = SWEEP + SPLIT_CASES


def gup(t):
    return torch.tensor(G_UP, dtype=torch.float64, device=t.device)


def ids(cases):
    return ["-".join(str(round(x, 4) if isinstance(x, float) else x) for x in c) for c in cases]


# ------------------------------------------------------------------------------------------------ one call, against the mirror
def pair_call(ops, a, b, positive, tau, backward=True):
    """Forward and (by default) backward on the device: Z and Zc, the loss, the rows, ga, gb; the forward's parts and groups."""
    ta, tb = torch.from_numpy(a).cuda().requires_grad_(backward), torch.from_numpy(b).cuda().requires_grad_(backward)
    z = forward_z(ops, ta.detach(), tb.detach(), tau, positive)
    loss, rows = ops.info_nce_pair(ta, tb, tau=tau, positive=positive, return_rows=True)
    st = dict(ops.last_stats)
    assert st["host_syncs"] == 0 and (st["rows"], st["features"]) == a.shape
    out = {"z": z, "loss": loss.detach(), "rows": rows, "parts": st["parts"], "groups": st["groups"]}
    if backward:
        loss.backward(gup(loss))
        assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["rows"] == a.shape[0]
        out["ga"], out["gb"] = ta.grad, tb.grad
    return out


def pair_case(ops, mirror, n, f, positive, tau):
    a, b = views(n, f)
    m = mirror(n, f, positive, tau)
    out = pair_call(ops, a, b, positive, tau)
    assert (out["parts"], out["groups"]) == (mirror.lib.pair_parts(n), mirror.lib.pair_groups(n))
    z = out["z"].cpu().numpy()
    assert bits(z[0]) == bits(m["z"][0]), "Z" + where(z[0], m["z"][0])
    assert bits(z[1]) == bits(m["z"][1]), "Zc" + where(z[1], m["z"][1])
    err = rows_against_the_mirror(out["rows"], m, positive, tau)
    print(f"pair n={n} F={f} {positive} tau={tau}: rows max |diff| {err:.3g}, loss diff {abs(float(out['loss']) - m['loss']):.3g}")
    assert err <= 1e-13
    assert abs(float(out["loss"]) - m["loss"]) <= 1e-13
    assert bits(out["ga"]) == bits(m["ga"]), "ga" + where(out["ga"].cpu().numpy(), m["ga"])
    assert bits(out["gb"]) == bits(m["gb"]), "gb" + where(out["gb"].cpu().numpy(), m["gb"])
    return out


# ------------------------------------------------------------------------------------------------ a, b: against the mirror
@pytest.mark.parametrize("n,f,positive,tau", SWEEP, ids=ids(SWEEP))
def test_feature_sweep(ops, mirror, n, f, positive, tau):
    pair_case(ops, mirror, n, f, positive, tau)


@pytest.mark.parametrize("n,f,positive,tau", SPLIT_CASES, ids=ids(SPLIT_CASES))
def test_work_split_edges(ops, mirror, n, f, positive, tau):
    out = pair_case(ops, mirror, n, f, positive, tau)
    assert (out["parts"], out["groups"], mirror.lib.pair_span_tiles(n)) == SPLIT_WANT[n]


# ------------------------------------------------------------------------------------------------ c, d: the host statements
def expw_of(lib1, tau):
    """The three values of e on the exact data, as float32: expw((s - 1) * (float)(1 / tau)) for s = -0.5, 0, 0.5."""
    itf = np.float32(1.0 / tau)
    return {v: im.expw(lib1, np.array([(np.float32(v) - np.float32(1.0)) * itf], dtype=np.float32))[0] for v in (-0.5, 0.0, 0.5)}


def leading_similarities(b, m=64):
    """s_ij = bh_j[i mod F] of the exact data for i, j < m: a corner of S, which shows S != S^T without the N x N matrix."""
    f = b.shape[1]
    return (b[:m] / 2.0)[:, np.arange(m) % f].T


def pair_counts(lib1, b, tau, positive):
    """Z, Zc, both row lists and the loss on exact data (exact_views, pm.exact_views_fast), in O(N F): a_i = e_(i mod F) has norm 1
    and b_j norm 2, so ah = a, bh = b / 2 and s_ij = bh_j[i mod F] exactly -- 0 or +-0.5, the same for every anchor i of a class.
      z[0]   Z_i of a class: over the columns j, a count of the three expw values;
      z[1]   Zc_j: over the anchors i, the count of value v is the number of anchors whose class holds v in column j;
    the float64 sums of these 24-bit values are exact in any order (the callers say why at their tau and N), so these are the float64
    values the rule gives.  rows: c s_ii - 1 / tau - log of each, s_ii = bh_i[i mod F]; the loss from math.fsum means."""
    n, f = b.shape
    cls = np.arange(n) % f
    S = (b.astype(np.float64) / 2.0).T.copy()                                  # S[c, j] = s_ij of every i of class c
    assert np.isin(S, (-0.5, 0.0, 0.5)).all()
    count = np.bincount(cls, minlength=f)                                      # the anchors of each class
    e = {v: np.float64(x) for v, x in expw_of(lib1, tau).items()}
    z = sum((S == v).sum(axis=1) * e[v] for v in (-0.5, 0.0, 0.5))[cls]
    zc = sum(((S == v) * count[:, None]).sum(axis=0) * e[v] for v in (-0.5, 0.0, 0.5))
    c = 1.0 if positive == "raw" else 1.0 / tau
    sii = S[cls, np.arange(n)]
    rows = np.stack([c * sii - 1.0 / tau - np.log(z), c * sii - 1.0 / tau - np.log(zc)])
    loss = -0.5 * (math.fsum(rows[0]) / n + math.fsum(rows[1]) / n)
    return {"z": np.stack([z, zc]), "rows": rows, "loss": loss, "S": S, "count": count}


def pair_by_class(lib1, b, tau, positive, g):
    """pair_counts and a float64 statement of both gradients, no rule: with the row softmax P_cj = exp(s_cj / tau) / sum_j' exp(s_cj'
    / tau) and the column softmax Q_cj = exp(s_cj / tau) / sum_i exp(s_(class i),j / tau),
      d loss / d ah_i = -(g / (2 N)) (2 c bh_i - (1 / tau) sum_j (P + Q)_(class i),j bh_j),
      d loss / d bh_j = -(g / (2 N)) (2 c ah_j - (1 / tau) sum_i (P + Q)_(class i),j ah_i), the inner sum being count_k (P + Q)_kj in
    column k, both pushed through the normalisation x -> x / |x| (norms 1 and 2)."""
    n, f = b.shape
    out = pair_counts(lib1, b, tau, positive)
    S, count, cls = out["S"], out["count"], np.arange(n) % f
    bh = b.astype(np.float64) / 2.0
    ah = np.zeros((n, f))
    ah[np.arange(n), cls] = 1.0
    X = np.exp(S / tau)
    W = X / X.sum(axis=1, keepdims=True) + X / (count[:, None] * X).sum(axis=0, keepdims=True)
    c = 1.0 if positive == "raw" else 1.0 / tau
    gs = -(g / (2.0 * n))
    Ga = gs * (2.0 * c * bh - (W @ bh)[cls] / tau)
    Gb = gs * (2.0 * c * ah - (count[:, None] * W).T / tau)
    out["ga"] = (Ga - ah * (ah * Ga).sum(axis=1, keepdims=True)) / 1.0
    out["gb"] = (Gb - bh * (bh * Gb).sum(axis=1, keepdims=True)) / 2.0
    return out


def pair_rule_by_class(lib1, b, tau, positive, g):
    """ga, gb of rlap_infonce.h's pair rule on the same data, bit for bit, in O(N^2 / F) vectorised work: what the pair's mirror would
    give had it the time.  w_ij = pair_weight(e_ij, rza_i, rzb_j) = e (rza + rzb) in float32 takes one value per (class of i, j), and
    every product of the chains is exact (bh is 0 or +-0.5, ah is 0 or 1), so a step fmaf(w, x, acc) is the float32 sum acc + w x, or
    acc where x = 0:
      D    of an anchor depends on its class alone: F chains over the samples in the header's order (the parts of infonce::num_parts,
           tiles, registers, halves), F columns each;
      D'   of sample j in column k adds w_kj once per anchor of class k in the part, whatever their order;
    then the float64 push through the normalisation with the header's operations in their order (pair_grad_scale, pair_positive_coef,
    grad_hat, dot_step, grad_in; norms 1 and 2, never clamped)."""
    n, f = b.shape
    cls = np.arange(n) % f
    bh = (b / np.float32(2.0)).astype(np.float32)
    S = bh.T.copy()
    e = expw_of(lib1, tau)
    e32 = np.zeros((f, n), dtype=np.float32)
    for v in (-0.5, 0.0, 0.5):
        e32[S == np.float32(v)] = e[v]
    count_all = np.bincount(cls, minlength=f)
    z = e32.astype(np.float64).sum(axis=1)                                      # by class; exact in any order
    zc = (count_all[:, None] * e32.astype(np.float64)).sum(axis=0)              # by column; exact in any order
    rza, rzb = (1.0 / z).astype(np.float32), (1.0 / zc).astype(np.float32)      # recip_z
    W = e32 * (rza[:, None] + rzb[None, :])                                     # (F, N) float32: pair_weight
    assert W.dtype == np.float32
    parts = lib1.infonce_parts(n)
    begin = [lib1.infonce_part_begin(n, p) for p in range(parts + 1)]
    order = [lib1.infonce_reg_row(r, h) for r in range(16) for h in range(2)]
    D = np.zeros((f, f), dtype=np.float32)                                      # [class, column]
    Dp = np.zeros((n, f), dtype=np.float32)
    WT = np.ascontiguousarray(W.T)                                              # [j, k]
    for p in range(parts):
        acc = np.zeros((f, f), dtype=np.float32)
        for t in range(begin[p], begin[p + 1]):
            for o in order:
                j = 32 * t + o
                if j < n:
                    acc = acc + W[:, j, None] * bh[None, j, :]
        D = D + acc
        lo, hi = 32 * begin[p], min(n, 32 * begin[p + 1])
        count = np.bincount(cls[lo:hi], minlength=f)                            # the part's anchors of each class
        accp = np.zeros((n, f), dtype=np.float32)
        for step in range(count.min()):
            accp += WT
        for step in range(count.min(), count.max()):
            accp = np.where((step < count)[None, :], accp + WT, accp)
        Dp = Dp + accp
    assert D.dtype == np.float32 and Dp.dtype == np.float32
    ah = np.zeros((n, f), dtype=np.float32)
    ah[np.arange(n), cls] = 1.0
    c2, itau, gs2 = 2.0 * (1.0 if positive == "raw" else 1.0 / tau), 1.0 / tau, -(g / (2.0 * float(n)))

    def push(own, other, chain, nrm):
        G = gs2 * (c2 * other.astype(np.float64) - itau * chain.astype(np.float64))
        dot = np.zeros(n)
        for k in range(f):
            dot = dot + own[:, k].astype(np.float64) * G[:, k]
        return ((G - own.astype(np.float64) * dot[:, None]) / nrm).astype(np.float32)
    return {"ga": push(ah, bh, D[cls], 1.0), "gb": push(bh, ah, Dp, 2.0)}


def grad_rel(ga, gb, want):
    """The largest difference of either gradient, relative to the largest entry of both (as tests/test_infonce_pair_cpu.py)."""
    gmax = max(np.abs(want["ga"]).max(), np.abs(want["gb"]).max())
    return max(np.abs(ga - want["ga"]).max(), np.abs(gb - want["gb"]).max()) / gmax


def loss_bound(n, rows):
    """|a sum of N float64 terms in any order - the exact sum| <= (N - 1) 2^-53 sum |terms| to first order, so the mean moves by at
    most N 2^-53 max |row|; twice that covers the second-order term, the last place of each row and the final operations."""
    return n * 2.0 ** -52 * np.abs(rows).max()


def timed(call):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = call()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def test_single_part_backward(ops, mirror):
    """Measured on an MI355X: the device calls (the forward twice, the backward once) 0.014 s together; the test 0.8 s, most of it the
    two host statements."""
    from test_infonce_pair_regimes_cpu import SINGLE_PART_GRAD_BOUND           # measured on the CPU, never from a device run
    n, f, positive, tau = SINGLE_PART
    lib1 = mirror.lib1
    assert lib1.infonce_parts(n) == 1 and lib1.infonce_parts(n - 1) == 2       # the first N of the regime
    a, b = exact_views(n, f)
    assert not np.array_equal(leading_similarities(b), leading_similarities(b).T)
    # 24-bit values below 1 within two binades (e^-0.75 .. e^-0.25), at most 2^15 of them: every partial sum is a multiple of 2^-26
    # below 2^15, exact in float64 in any order
    want = pair_by_class(lib1, b, tau, positive, G_UP)
    assert np.median(np.abs(want["z"][0] - want["z"][1]) / want["z"][0]) > 0.05   # a swap of rows and columns would show
    out, seconds = timed(lambda: pair_call(ops, a, b, positive, tau))
    assert (out["parts"], out["groups"]) == (mirror.lib.pair_parts(n), mirror.lib.pair_groups(n)) == (32, 16)
    z = out["z"].cpu().numpy()
    assert bits(z[0]) == bits(want["z"][0]), "Z" + where(z[0], want["z"][0])
    assert bits(z[1]) == bits(want["z"][1]), "Zc" + where(z[1], want["z"][1])
    err = np.abs(out["rows"].cpu().numpy() - want["rows"]).max()
    dl = abs(float(out["loss"]) - want["loss"])
    rel = grad_rel(out["ga"].cpu().numpy().astype(np.float64), out["gb"].cpu().numpy().astype(np.float64), want)
    print(f"pair n={n} F={f} {positive} tau={tau}, one backward part, {seconds:.3f} s: rows max |diff| {err:.3g}, loss diff {dl:.3g} "
          f"(bound {loss_bound(n, want['rows']):.3g}), gradients rel {rel:.3g} (bound {SINGLE_PART_GRAD_BOUND:.3g})")
    assert err <= 1e-13                                                        # s_ii exact: the class's entry, not a neighbour's
    assert dl <= loss_bound(n, want["rows"])
    assert bool(torch.isfinite(out["ga"]).all()) and bool(torch.isfinite(out["gb"]).all())
    rule = pair_rule_by_class(lib1, b, tau, positive, G_UP)
    assert bits(out["ga"]) == bits(rule["ga"]), "ga" + where(out["ga"].cpu().numpy(), rule["ga"])
    assert bits(out["gb"]) == bits(rule["gb"]), "gb" + where(out["gb"].cpu().numpy(), rule["gb"])
    assert rel <= SINGLE_PART_GRAD_BOUND


def test_a_part_of_two_spans(ops, mirror):
    """Measured on an MI355X: the two forward calls (one for Z and Zc, one for the loss and the rows) 0.44 s together, copies of the
    inputs included; the test 0.5 s."""
    n, f, positive, tau = TWO_SPANS
    lib, lib1 = mirror.lib, mirror.lib1
    parts = lib.pair_parts(n)
    lengths = [lib.pair_part_begin(n, p + 1) - lib.pair_part_begin(n, p) for p in range(parts)]
    assert lib.pair_span_tiles(n) == lib.pair_span_cap() == 256 and max(lengths) > 256     # some part has a second span
    assert lib.pair_span_tiles(n - 1) == 256 and max(lib.pair_part_begin(n - 1, p + 1) - lib.pair_part_begin(n - 1, p) for p in range(parts)) == 256
    a, b = pm.exact_views_fast(n, f)
    assert not np.array_equal(leading_similarities(b), leading_similarities(b).T)
    # the three values span e^4 (e^-6 .. e^-2 at tau = 1/4), the sums stay below 2^16 and the smallest ulp is 2^-32: 48 bits, exact
    # in float64 in any order
    want = pair_counts(lib1, b, tau, positive)
    assert want["z"].max() < 2.0 ** 16 and min(expw_of(lib1, tau).values()) >= 2.0 ** -9
    assert np.median(np.abs(want["z"][0] - want["z"][1]) / want["z"][0]) > 0.05   # a swap of rows and columns would show
    out, seconds = timed(lambda: pair_call(ops, a, b, positive, tau, backward=False))
    assert (out["parts"], out["groups"]) == (parts, lib.pair_groups(n)) == (32, 16)
    z = out["z"].cpu().numpy()
    assert bits(z[0]) == bits(want["z"][0]), "Z" + where(z[0], want["z"][0])
    assert bits(z[1]) == bits(want["z"][1]), "Zc" + where(z[1], want["z"][1])
    err = np.abs(out["rows"].cpu().numpy() - want["rows"]).max()
    dl = abs(float(out["loss"]) - want["loss"])
    print(f"pair n={n} F={f} {positive} tau={tau}, a part of {max(lengths)} tiles, {seconds:.3f} s: rows max |diff| {err:.3g}, "
          f"loss diff {dl:.3g} (bound {loss_bound(n, want['rows']):.3g})")
    assert err <= 1e-13
    assert dl <= loss_bound(n, want["rows"])


# ------------------------------------------------------------------------------------------------ e: a poisoned arena
@pytest.mark.parametrize("n,f,positive,tau", POISON, ids=ids(POISON))
def test_partially_filled_with_a_poisoned_arena(ops, mirror, n, f, positive, tau):
    def call():
        return {k: bits(v) for k, v in pair_case(ops, mirror, n, f, positive, tau).items() if isinstance(v, torch.Tensor)}
    base = call()
    ops.debug_set_poison(0xFF)
    try:
        again = call()
    finally:
        ops.debug_set_poison(-1)
    assert sorted(again) == sorted(base) == ["ga", "gb", "loss", "rows", "z"]
    for key in base:
        assert again[key] == base[key], f"{key} depends on what the arena held"
