"""What tests/test_gpu_infonce_pair_regimes.py reaches, and the oracles of its two large cases, without a GPU.

  * the accounting: the case lists of that file fed through the rules the launchers call (infonce::main_instance, num_parts,
    pair_groups, pair_parts, pair_span_tiles, exported by the two mirror libraries): every (instance, tile count) of the backward
    ladder at both fills, each instance that can have dead tiles with and without them; parts == T and parts < T in both splits;
    fewer than 16 groups, 16 groups, a group of two row blocks; spans of 1, 2, 3 tiles, the cap of 256 and a part of two spans; the
    backward's single part.  Every list is also held to its members, so a case that is removed fails here;
  * pair_by_class, the O(N F) statement that the single-part case is held to (its counts are also the two-span case's), against the
    pair's mirror and against the autograd restatement on the same construction at N = 2708 (12 backward parts, 16 groups, groups of
    one and of two row blocks): Z and Zc bit for bit, the gradients within GRAD_BOUND of tests/test_infonce_pair_cpu.py;
    pair_rule_by_class, the rule's bits on that construction, against the mirror bit for bit;
  * SINGLE_PART_GRAD_BOUND, the bound of the single-part case's gradients against the float64 statement.  On that data a chain of
    32,641 float32 steps adds a few values again and again, so the rule's rounding is systematic and not that of GRAD_BOUND's random
    inputs; the device must add none of its own (it equals the rule bit for bit), so the bound is the rule's own distance from the
    statement, computed here on the CPU at N = 32,641: 4.395e-6 of the largest gradient entry.  The bound is four times that, the
    project's convention;
  * the vectorised exact-data generator of the two-span case.
"""
import numpy as np
import pytest

import infonce_mirror as im
import infonce_pair_mirror as pm
import test_gpu_infonce_pair_regimes as pr
from test_gpu_infonce_pair import exact_views
from test_infonce_pair_cpu import GRAD_BOUND

SINGLE_PART_RULE_REL = 4.395e-6                      # pair_rule_by_class against pair_by_class at SINGLE_PART, measured below
SINGLE_PART_GRAD_BOUND = 4 * SINGLE_PART_RULE_REL    # of the largest gradient entry


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("infonce_pair_regimes")
    return {"pair": pm.build(d), "one": im.build(d)}


def tiles(n):
    return (n + 31) // 32


def part_lengths(lib, n):
    return [lib.pair_part_begin(n, p + 1) - lib.pair_part_begin(n, p) for p in range(lib.pair_parts(n))]


def group_lengths(lib, n):
    return [lib.pair_group_begin(n, q + 1) - lib.pair_group_begin(n, q) for q in range(lib.pair_groups(n))]


# ------------------------------------------------------------------------------------------------ the accounting
def test_the_sweep_reaches_every_backward_instance_at_every_fill(libs):
    one = libs["one"]
    ladder = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8, **{t: 16 for t in range(9, 17)}}   # what the kernels were written for
    fs = [f for _, f, _, _ in pr.SWEEP]
    assert len(fs) == len(set(fs)) == 32
    # per tile count both fills: one live column in the last tile, and a full last tile (32 cases for 32 pairs: none to spare)
    assert {(one.infonce_feature_tiles(f), f % 32) for f in fs} == {(t, r) for t in range(1, 17) for r in (0, 1)}
    reached = {(one.infonce_main_instance(one.infonce_feature_tiles(f)), one.infonce_feature_tiles(f)) for f in fs}
    assert reached == {(ladder[t], t) for t in range(1, 17)}
    for inst in (4, 8, 16):                                                        # with dead accumulator tiles, and with none
        assert any(i == inst and t < inst for i, t in reached) and (inst, inst) in reached
    # the sweep's rows: two row blocks, the second with two live waves, a last tile with one live row
    assert {n for n, _, _, _ in pr.SWEEP} == {pr.SWEEP_N} and tiles(pr.SWEEP_N) == 6 and pr.SWEEP_N % 32 == 1
    # both settings of the positive term and the three values of tau take turns
    assert {p for _, _, p, _ in pr.SWEEP} == set(pr.POSITIVES) and {t for _, _, _, t in pr.SWEEP} == set(pr.TAUS)
    # the poisoned cases: nft 3 in instance 4 (one dead tile), nft 9 in instance 16 (seven)
    dead = [(one.infonce_main_instance(one.infonce_feature_tiles(f)), one.infonce_feature_tiles(f)) for _, f, _, _ in pr.POISON]
    assert dead == [(4, 3), (16, 9)] and all(n == pr.SWEEP_N for n, _, _, _ in pr.POISON)


def test_the_split_table_is_the_header_s(libs):
    lib, one = libs["pair"], libs["one"]
    assert [n for n, _, _, _ in pr.SPLIT] == [1024, 1056, 1408, 1409, 1920, 1921, 2048, 2049] == [n for n, _, _, _ in pr.SPLIT_CASES]
    assert all(f == 3 for _, f, _, _ in pr.SPLIT_CASES)
    for n, parts, groups, span in pr.SPLIT:
        assert (lib.pair_parts(n), lib.pair_groups(n), lib.pair_span_tiles(n)) == (parts, groups, span), n
        assert max(part_lengths(lib, n)) == span and sum(part_lengths(lib, n)) == tiles(n)
    # the backward's parts: == T at 1024, < T from 1056 on
    assert (one.infonce_parts(1024), tiles(1024)) == (32, 32) and (one.infonce_parts(1056), tiles(1056)) == (29, 33)
    # the forward: one tile per part and one row block per group up to 1408 ...
    assert max(n for n in range(1, 2100) if lib.pair_parts(n) == tiles(n)) == 1408
    assert (lib.pair_parts(1056), lib.pair_groups(1056)) == (33, 9) and (lib.pair_parts(1408), lib.pair_groups(1408)) == (44, 11)
    # ... then parts of one and two tiles below T, the last row block with one live wave of one live row
    assert (lib.pair_parts(1409), tiles(1409)) == (43, 45) and set(part_lengths(lib, 1409)) == {1, 2}
    assert tiles(1409) % 4 == 1 and 1409 % 32 == 1 and set(group_lengths(lib, 1409)) == {1}
    assert (lib.pair_groups(1920), lib.pair_parts(1920)) == (15, 35) and set(part_lengths(lib, 1920)) == {1, 2}
    # the first N of 16 groups
    assert min(n for n in range(1, 2100) if lib.pair_groups(n) == 16) == 1921 and tiles(1921) == 61 and set(part_lengths(lib, 1921)) == {1, 2}
    # all parts two tiles, all blocks full; then the first group of two row blocks, parts of two and three tiles
    assert set(part_lengths(lib, 2048)) == {2} and set(group_lengths(lib, 2048)) == {1} and 2048 % 128 == 0
    assert min(n for n in range(1, 2100) if max(group_lengths(lib, n)) == 2) == 2049
    assert set(part_lengths(lib, 2049)) == {2, 3} and sorted(set(group_lengths(lib, 2049))) == [1, 2] and tiles(2049) % 4 == 1 and 2049 % 32 == 1


def test_the_cases_reach_every_regime_of_both_splits(libs):
    lib, one = libs["pair"], libs["one"]
    ns = [n for n, _, _, _ in pr.CASES] + [pr.SINGLE_PART[0], pr.TWO_SPANS[0]]
    both = {"== T", "< T"}
    assert {"== T" if one.infonce_parts(n) == tiles(n) else "< T" for n, _, _, _ in pr.CASES} == both      # the backward's split
    assert {"== T" if lib.pair_parts(n) == tiles(n) else "< T" for n, _, _, _ in pr.CASES} == both         # the forward's
    groups = {lib.pair_groups(n) for n in ns}
    assert min(groups) < 16 and max(groups) == 16
    assert any(lib.pair_groups(n) == 16 and set(group_lengths(lib, n)) == {1} for n in ns)                 # 16 groups of one block
    assert any(max(group_lengths(lib, n)) == 2 for n, _, _, _ in pr.CASES)                                 # a two-block group
    spans = {lib.pair_span_tiles(n) for n in ns}
    assert {1, 2, 3, 256} <= spans and lib.pair_span_cap() == 256
    # the backward's single part, at the first N that has it, with the workloads' forward split; the workloads are in this regime
    n = pr.SINGLE_PART[0]
    assert one.infonce_parts(n) == 1 and one.infonce_parts(n - 1) == 2 and n == 32641
    assert one.infonce_parts(34493) == 1 and one.infonce_parts(169343) == 1
    assert max(one.infonce_parts(m) for m, _, _, _ in pr.CASES) > 1
    assert (lib.pair_parts(n), lib.pair_groups(n)) == (lib.pair_parts(169343), lib.pair_groups(169343)) == (32, 16)
    # a part of two spans, at the first N that has one: one part of 257 tiles, whose last tile holds one live row
    n = pr.TWO_SPANS[0]
    assert n == 262145 and tiles(n) == 8193 and n % 32 == 1
    assert sorted(part_lengths(lib, n)) == [256] * 31 + [257] and max(part_lengths(lib, n - 1)) == 256
    assert max(max(part_lengths(lib, m)) for m in ns if m != n) <= 256                                     # and no other case has one
    assert pr.SINGLE_PART[1:] == (8, "raw", 2.0) and pr.TWO_SPANS[1:] == (8, "raw", 0.25)


# ------------------------------------------------------------------------------------------------ the host statements
def test_the_statements_by_class_agree_with_the_mirror_and_with_autograd(libs):
    """pair_by_class and pair_rule_by_class on the construction of the single-part case, at a size where the O(N^2) oracles run."""
    n, (_, f, positive, tau) = 2708, pr.SINGLE_PART
    lib, one = libs["pair"], libs["one"]
    assert one.infonce_parts(n) == 12 and lib.pair_groups(n) == 16 and sorted(set(group_lengths(lib, n))) == [1, 2]
    a, b = exact_views(n, f)
    want = pr.pair_by_class(one, b, tau, positive, pr.G_UP)
    m = pm.run(lib, a, b, tau, positive, g=pr.G_UP)
    loss, ga, gb = pm.restatement(a, b, tau, positive, g=pr.G_UP)
    assert m["z"][0].tobytes() == want["z"][0].tobytes()                           # the counts are the rule's Z and Zc, bit for bit
    assert m["z"][1].tobytes() == want["z"][1].tobytes()
    assert np.median(np.abs(want["z"][0] - want["z"][1]) / want["z"][0]) > 0.05
    assert np.abs(m["rows"] - want["rows"]).max() <= 1e-13
    rel_mirror = pr.grad_rel(m["ga"].astype(np.float64), m["gb"].astype(np.float64), want)
    rel_auto = pr.grad_rel(ga, gb, want)
    print(f"pair by class at n={n} F={f}: mirror rel {rel_mirror:.3g}, autograd rel {rel_auto:.3g}, loss: mirror diff {abs(m['loss'] - want['loss']):.3g}, "
          f"autograd diff {abs(loss - want['loss']):.3g}")
    assert rel_mirror <= GRAD_BOUND
    assert rel_auto <= GRAD_BOUND
    assert abs(m["loss"] - want["loss"]) <= pr.loss_bound(n, want["rows"])
    rule = pr.pair_rule_by_class(one, b, tau, positive, pr.G_UP)
    assert rule["ga"].tobytes() == m["ga"].tobytes(), "ga" + pr.where(rule["ga"], m["ga"])
    assert rule["gb"].tobytes() == m["gb"].tobytes(), "gb" + pr.where(rule["gb"], m["gb"])


def test_the_counts_agree_with_the_mirror_on_the_vectorised_data(libs):
    """pair_counts on pm.exact_views_fast at the two-span case's F and tau, where the mirror runs: N = 2049 (groups of one and of two
    row blocks, parts of two and three tiles)."""
    n, (_, f, positive, tau) = 2049, pr.TWO_SPANS
    a, b = pm.exact_views_fast(n, f)
    want = pr.pair_counts(libs["one"], b, tau, positive)
    m = pm.run(libs["pair"], a, b, tau, positive)
    assert m["z"][0].tobytes() == want["z"][0].tobytes() and m["z"][1].tobytes() == want["z"][1].tobytes()
    assert np.abs(m["rows"] - want["rows"]).max() <= 1e-13
    assert abs(m["loss"] - want["loss"]) <= pr.loss_bound(n, want["rows"])


def test_the_measured_bound_of_the_single_part_case(libs):
    """The rule against the float64 statement at N = 32,641, F = 8, raw, tau = 2: 4.395e-6 of the largest gradient entry, measured
    here (SINGLE_PART_RULE_REL); the GPU test is held to four times that."""
    n, f, positive, tau = pr.SINGLE_PART
    _, b = exact_views(n, f)
    want = pr.pair_by_class(libs["one"], b, tau, positive, pr.G_UP)
    rule = pr.pair_rule_by_class(libs["one"], b, tau, positive, pr.G_UP)
    rel = pr.grad_rel(rule["ga"].astype(np.float64), rule["gb"].astype(np.float64), want)
    print(f"the rule against the float64 statement at n={n} F={f} {positive} tau={tau}: gradients rel {rel:.4g}")
    assert np.isfinite(rule["ga"]).all() and np.isfinite(rule["gb"]).all()
    assert rel <= SINGLE_PART_RULE_REL * 1.005                                     # the figure stated above is the one measured
    assert rel >= SINGLE_PART_RULE_REL * 0.995
    assert SINGLE_PART_GRAD_BOUND == 4 * SINGLE_PART_RULE_REL


# ------------------------------------------------------------------------------------------------ the vectorised generator
@pytest.mark.parametrize("n,f", [(300, 8), (2049, 8), (129, 33), pr.TWO_SPANS[:2]])
def test_the_vectorised_generator_gives_exact_data(n, f):
    a, b = pm.exact_views_fast(n, f)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (n, f)
    assert np.array_equal((a.astype(np.float64) ** 2).sum(axis=1), np.ones(n))                 # rows of norm 1
    assert np.array_equal(a.argmax(axis=1), np.arange(n) % f) and (a != 0).sum() == n          # a_i = e_(i mod F)
    assert np.array_equal((b.astype(np.float64) ** 2).sum(axis=1), np.full(n, 4.0))            # rows of norm 2 ...
    assert np.isin(b, (-1.0, 0.0, 1.0)).all() and np.array_equal((b != 0).sum(axis=1), np.full(n, 4))   # ... of four entries +-1
    m = min(n, 256)
    s = pr.leading_similarities(b, m)                                                          # s_ij = bh_j[i mod F]
    ah, bh = a[:m].astype(np.float64), b[:m].astype(np.float64) / 2.0
    assert np.array_equal(s, ah @ bh.T)
    assert np.isin(s, (-0.5, 0.0, 0.5)).all() and {-0.5, 0.0, 0.5} == set(np.unique(s))
    assert not np.array_equal(s, s.T)
    # both signs and every column are used about evenly: the margin between Z and Zc rests on it
    assert abs((b == 1).sum() - (b == -1).sum()) <= 8 * np.sqrt(n) and (b != 0).sum(axis=0).min() >= 2 * n // f
    b2 = pm.exact_views_fast(n, f)[1]
    assert np.array_equal(b, b2)                                                               # the same draws every time
