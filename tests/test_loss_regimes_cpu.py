"""What tests/test_gpu_loss_regimes.py reaches, and the oracle of its single-part case, without a GPU.

  * the accounting: the case lists of that file fed through the rules the launchers call (infonce::main_instance, cca::gram_instance,
    cca::zr_instance, g2l::vec_rows and the three num_parts, exported by the mirror libraries): every (instance, tile count) of the
    five template ladders, every count of pair groups and of live waves in the last one, every value of vec_rows on both sides of
    each edge, parts == T and parts < T in every family, and InfoNCE's single part.  If a rule changes and the cases stop covering
    it, this fails;
  * by_class, the O(N F) float64 statement that the single-part case is held to, against the mirror and against the autograd
    restatement on the same construction at N = 2708, within GRAD_BOUND / 4; rule_by_class, the rule's bits on that construction,
    against the mirror bit for bit.
"""
import numpy as np
import pytest

import cca_mirror as cm
import g2l_mirror as gm
import infonce_mirror as im
import test_gpu_loss_regimes as lr
from test_gpu_infonce import exact_views
from test_infonce_cpu import GRAD_BOUND


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("loss_regimes")
    return {"in": im.build(d), "cca": cm.build(d), "g2l": gm.build(d)}


def tiles(n):
    return (n + 31) // 32


def test_the_cases_reach_every_instance_at_every_fill(libs):
    ladder = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8, **{t: 16 for t in range(9, 17)}}   # what the kernels were written for
    every = {(ladder[t], t) for t in range(1, 17)}

    def reached(tiles_of, instance_of, fs):
        # per tile count both fills: one live column in the last tile, and a full last tile
        assert {(tiles_of(f), f % 32) for f in fs} >= {(t, r) for t in range(1, 17) for r in (0, 1)}
        return {(instance_of(tiles_of(f)), tiles_of(f)) for f in fs}

    lin, lcca, lg = libs["in"], libs["cca"], libs["g2l"]
    # k_in_main (both backward modes run in every call), k_g2l_main dh and dg (G >= 2), k_cca_gram, k_cca_zr
    assert reached(lin.infonce_feature_tiles, lin.infonce_main_instance, [f for _, f, _, _ in lr.INFONCE_SWEEP]) == every
    many = [f for _, G, f, _ in lr.JSD_MANY_SWEEP if G >= 2]
    assert reached(lg.g2l_feature_tiles, lg.g2l_main_instance, many) == every      # dh: the nodes own; dg: the graphs own
    assert reached(lcca.cca_feature_tiles, lcca.cca_gram_instance, [f for _, f, _ in lr.CCA_SWEEP]) == every
    zr = reached(lcca.cca_feature_tiles, lcca.cca_zr_instance, [f for _, f, _ in lr.CCA_SWEEP])
    assert zr == {((t + 3) // 4, t) for t in range(1, 17)}
    assert {t % 4 for _, t in zr} == {0, 1, 2, 3}                                  # waves that own different numbers of column tiles
    # the sweep's rows: two row blocks, the second with two live waves, a last tile with one live row, an odd N
    assert tiles(lr.SWEEP_N) == 6 and lr.SWEEP_N % 32 == 1 and lr.SWEEP_N % 2 == 1
    # no instance outside the tile counts of a call
    assert lin.infonce_main_instance(0) == lin.infonce_main_instance(17) == lcca.cca_gram_instance(17) == lcca.cca_zr_instance(0) == 0


def test_the_cases_reach_every_pair_group_count(libs):
    lib = libs["cca"]
    fs = [f for _, f, _ in lr.CCA_CASES]
    assert {lib.cca_pair_groups(f) for f in fs} == {lib.cca_pair_groups(f) for f in range(1, 513)} == {1, 2, 3, 4, 6, 7, 9}
    assert {lib.cca_super_pairs(f) % 4 for f in fs} == {0, 1, 2, 3}                # live waves of the last group: 4, 1, 2, 3
    odd = {lib.cca_feature_tiles(f) for f in fs if lib.cca_feature_tiles(f) % 2}  # a clamped tile: computed twice, stored once
    assert odd == {1, 3, 5, 7, 9, 11, 13, 15}
    assert (lib.cca_pair_groups(161), lib.cca_super_pairs(161)) == (2, 6)          # nft 6: two groups, two live waves
    assert (lib.cca_pair_groups(353), lib.cca_super_pairs(353)) == (6, 21)         # nft 12: six groups, one live wave
    assert lr.POISON_CCA[1] == 161


def test_the_cases_reach_every_vec_rows_value_on_both_sides_of_each_edge(libs):
    lib = libs["g2l"]
    edges = [f for f in range(1, 512) if lib.g2l_vec_rows(f) != lib.g2l_vec_rows(f + 1)]
    assert [(f, lib.g2l_vec_rows(f), lib.g2l_vec_rows(f + 1)) for f in edges] == [(65, 256, 128), (131, 128, 64), (263, 64, 32)]
    for cases in (lr.JSD_ONE_VEC, lr.BOOT_VEC):
        fs = {f for _, _, f, _ in cases}
        assert all(f in fs and f + 1 in fs for f in edges)
        for n, G, f, _ in cases:                                                   # several blocks, the last with one row
            assert lib.g2l_vec_blocks(n, f) >= 3 and n % lib.g2l_vec_rows(f) == 1
        assert {lib.g2l_vec_blocks(n, f) for n, _, f, _ in cases} == {3, 5, 9, 17}
    assert all(G == 1 for _, G, _, _ in lr.JSD_ONE_VEC) and all(G >= 2 for _, G, _, _ in lr.BOOT_VEC)


def test_the_cases_reach_both_part_regimes(libs):
    lin, lcca, lg = libs["in"], libs["cca"], libs["g2l"]

    def regimes(parts_and_tiles):
        return {"== T" if p == t else "< T" for p, t in parts_and_tiles}

    both = {"== T", "< T"}
    assert regimes((lin.infonce_parts(n), tiles(n)) for n, _, _, _ in lr.INFONCE_CASES) == both
    assert regimes((lcca.cca_parts(n, f), tiles(n)) for n, f, _ in lr.CCA_CASES) == both
    assert regimes((lg.g2l_parts(n, G, f), tiles(n)) for n, G, f, _ in lr.JSD_MANY_CASES) == both
    assert regimes((lg.g2l_parts(n, G, f), tiles(n)) for n, G, f, _ in lr.JSD_ONE_CASES) == both
    # the cases of section c, as the issue of the regime pass states them
    assert (lg.g2l_parts(4129, 129, 33), tiles(4129), tiles(129)) == (128, 130, 5) and (4129, 129, 33, "even") in lr.JSD_MANY_CASES
    sizes = {lg.g2l_part_begin(4129, 129, 33, p + 1) - lg.g2l_part_begin(4129, 129, 33, p) for p in range(128)}
    assert sizes == {1, 2}                                                         # uneven parts
    assert (lg.g2l_parts(32801, 1, 3), tiles(32801)) == (1024, 1026) and (32801, 1, 3, None) in lr.JSD_ONE_CASES
    assert (lcca.cca_parts(1000, 500), tiles(1000), lcca.cca_pair_groups(500)) == (29, 32, 9) and 500 % 32 != 0
    assert (lin.infonce_parts(1024), tiles(1024)) == (32, 32) and (lin.infonce_parts(1056), tiles(1056)) == (29, 33)
    assert {n for n, _, _, _ in lr.INFONCE_PARTS} == {1024, 1056}
    # InfoNCE: the single part, at the first N that has it; the workloads of tests/test_infonce_cpu.py are in the same regime
    n = lr.SINGLE_PART[0]
    assert lin.infonce_parts(n) == 1 and lin.infonce_parts(n - 1) == 2 and tiles(n) > 1
    assert lin.infonce_parts(34493) == 1 and lin.infonce_parts(169343) == 1
    assert max(lin.infonce_parts(n) for n, _, _, _ in lr.INFONCE_CASES) > 1


def test_the_statement_by_class_agrees_with_the_mirror_and_with_autograd(libs):
    """by_class on the construction of the single-part case, at a size where the O(N^2) oracles run: N = 2708 (twelve parts)."""
    n, (_, f, positive, tau) = 2708, lr.SINGLE_PART
    a, b = exact_views(n, f)
    want = lr.by_class(libs["in"], b, tau, positive, lr.G_UP)
    m = im.run(libs["in"], a, b, tau, positive, g=lr.G_UP)
    loss, ga, gb = im.restatement(a, b, tau, positive, g=lr.G_UP)
    assert m["z"].tobytes() == want["z"].tobytes()                                 # the count per class is the rule's Z, bit for bit
    assert np.abs(m["rows"] - want["rows"]).max() <= 1e-13
    rel_mirror = lr.grad_rel(m["ga"].astype(np.float64), m["gb"].astype(np.float64), want)
    rel_auto = lr.grad_rel(ga, gb, want)
    print(f"by class at n={n} F={f}: mirror rel {rel_mirror:.3g}, autograd rel {rel_auto:.3g}, loss diff {abs(loss - want['loss']):.3g}")
    assert rel_mirror <= GRAD_BOUND / 4
    assert rel_auto <= GRAD_BOUND / 4
    # rule_by_class, the rule's bits in O(N^2 / F): the mirror's, here through twelve parts
    assert libs["in"].infonce_parts(n) == 12
    rule = lr.rule_by_class(libs["in"], b, tau, positive, lr.G_UP)
    assert rule["ga"].tobytes() == m["ga"].tobytes() and rule["gb"].tobytes() == m["gb"].tobytes()
