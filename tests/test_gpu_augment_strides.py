"""The second round of every strided launch of the three augmentor calls (ops.drop_edges, ops.sample_subgraphs, ops.add_edges;
DESIGN 4.20 to 4.22).  A strided launch is capped at 8,192 workgroups of 256 lanes, MAX_GRID_ROWS = 2^21 items a round (the CPU
suites tie the constant to ED_MAX_GRID, NS_MAX_GRID, EA_MAX_GRID and TILE), so no loop `for (i = ...; i < n; i += gridDim.x * TILE)`
runs twice on fewer items: the other GPU files stop near 6,000 rows.  The input here is E = 2^21 + 65 random rows on N = 2^21 + 300
nodes: one full round, then one whole wave and one lane, so the second round holds a full wave, a wave with a single live lane and
workgroups with none -- what the loops that keep whole waves in them (k_ed_keys, k_ed_heads, k_ed_pr_gather with their ballots and
butterflies) and the wave reductions behind loops of unequal trip counts (ea_count) have to get right.  Every test asserts from the
sizes alone that the launches it is aimed at need a second round, then compares with the host mirror as the other GPU files do:
bit for bit, node_weight within the project's bound, one host synchronisation a call.  One test a call and scheme, a few seconds
each; most of that is the mirror on the host."""
import numpy as np
import pytest
import torch

import edge_add_cases as add_cases
import edge_drop_cases as cases
import edgeadd_mirror
import edgedrop_mirror
import node_sample_cases as sample_cases
import nodesample_mirror
from test_gpu_edge_drop_regimes import against_the_mirror

pytestmark = pytest.mark.gpu
ROUND = cases.MAX_GRID_ROWS


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def large():
    """(src, dst, n, edge_index on the device): made once, never written."""
    src, dst, n = cases.stride_rows()
    assert src.size == ROUND + 64 + 1
    return src, dst, n, torch.from_numpy(np.stack([src, dst])).cuda()


@pytest.fixture(scope="module")
def drop_mirror(tmp_path_factory):
    return edgedrop_mirror.build(tmp_path_factory.mktemp("edgedrop_strides"))


@pytest.fixture(scope="module")
def sample_mirror(tmp_path_factory):
    return nodesample_mirror.build(tmp_path_factory.mktemp("nodesample_strides"))


@pytest.fixture(scope="module")
def add_mirror(tmp_path_factory):
    return edgeadd_mirror.build(tmp_path_factory.mktemp("edgeadd_strides"))


def rounds(items):
    """The trips of a strided launch's first lane over `items`."""
    return -(-items // ROUND)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("scheme", cases.SCHEMES)
def test_edge_drop(ops, drop_mirror, large, scheme):
    """k_ed_keys over E rows; degree: k_ed_heads over 2 E keys, k_ed_degree over N; pagerank and eigenvector: k_rc_bounds over E,
    k_ed_fill, k_ed_pr_share, k_ed_evc_finish over N, k_ed_pr_gather over 16 N lanes; wg_total over 8,194 partials: 33 trips."""
    src, dst, n, _ = large
    E = src.size
    assert rounds(E) == 2 and rounds(2 * E) == 3 and rounds(n) == 2 and rounds(16 * n) == 17
    node_tiles = -(-n // cases.NODE_TILE)
    assert node_tiles == 8194 and -(-node_tiles // cases.NODE_TILE) == 33
    against_the_mirror(ops, drop_mirror, "large input", src, dst, n, cases.weights(E), scheme, "sink", **cases.STRIDE_ITERS)


def same_sample(got, want):
    ok = np.array_equal(bits(got[0].cpu().numpy()), bits(want["rows"])) and got[1].tolist() == want["ptr"].tolist()
    ok = ok and got[2].dtype == torch.bool and np.array_equal(got[2].cpu().numpy(), want["nodes"])
    if len(got) > 3:
        ok = ok and got[3].dtype == torch.int64 and np.array_equal(got[3].cpu().numpy(), want["walks"])
    return ok


def test_node_sample_drop(ops, sample_mirror, large):
    """k_ns_keys over E rows; k_ns_drop_bits over the bitmap's words, a wave a word and 4 a workgroup; k_ns_mask over K N bytes."""
    src, dst, n, ei = large
    words = -(-n // 64)
    assert rounds(src.size) == 2 and words > (ROUND // cases.NODE_TILE) * (cases.NODE_TILE // 64) and rounds(len(sample_cases.PS) * n) == 3
    want = nodesample_mirror.run(sample_mirror, src, dst, n, p=sample_cases.PS, seed=sample_cases.SEED)
    got = ops.sample_subgraphs(ei, None, n, "drop", list(sample_cases.PS), seed=sample_cases.SEED, return_nodes=True)
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["rows_needed"] == got[0].shape[0]
    assert same_sample(got, want) and 0 < got[0].shape[0] < 2 * src.size


def test_node_sample_walk(ops, sample_mirror, large):
    """k_ns_keys and k_rc_bounds over E rows; k_ns_walk over E + 3 walkers; k_ns_mask over K N bytes."""
    src, dst, n, ei = large
    E = src.size
    kw = dict(scheme="walk", num_seeds=[E, 3], walk_length=1, seed=sample_cases.SEED)
    assert rounds(E) == 2 and rounds(sum(kw["num_seeds"])) == 2 and rounds(2 * n) == 3
    want = nodesample_mirror.run(sample_mirror, src, dst, n, **kw)
    got = ops.sample_subgraphs(ei, None, n, return_nodes=True, return_walks=True, **kw)
    assert ops.last_stats["host_syncs"] == 1 and tuple(got[3].shape) == (E + 3, 2)
    assert same_sample(got, want) and (want["walks"][:, 0] != want["walks"][:, 1]).any() and got[0].shape[0] > 0


def add_both(ops, mirror, src, dst, n, w=None, **kw):
    """The call on the device and by the mirror, compared bit for bit as tests/test_gpu_edge_add.py compares them."""
    want = edgeadd_mirror.run(mirror, src, dst, n, w=w, **kw)
    ei = torch.from_numpy(np.stack([src, dst])).cuda()
    got = ops.add_edges(ei, None if w is None else torch.from_numpy(w).cuda(), n, return_added=True, **kw)
    st = dict(ops.last_stats)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(want["rows"])) and got[1].tolist() == want["ptr"].tolist()
    assert got[2].dtype == torch.int64 and np.array_equal(got[2].cpu().numpy(), want["added"]) and got[3].tolist() == want["aptr"].tolist()
    assert st["rows_needed"] == got[0].shape[0] and st["added"] == got[2].shape[0] and st["host_syncs"] == 1
    if kw.get("coalesce", True):
        assert st["input_sorted"] == want["input_sorted"] and st["input_distinct"] == want["input_distinct"]
    return got, want, st


def test_edge_add_large_input(ops, add_mirror, large):
    """k_ea_keys, k_ea_hash_insert (the key set: the rows are in no order), k_ea_heads_a and k_ea_runs_a over E rows, k_ea_hash_clear
    over 2 E slots; the rows as they stand (duplicates possible), general weights."""
    src, dst, n, _ = large
    E = src.size
    assert rounds(E) == 2 and rounds(E + 1) == 2 and rounds(2 * E) == 3
    got, want, st = add_both(ops, add_mirror, src, dst, n, w=add_cases.weights(E), ratio=[0.001], seed=add_cases.SEED)
    assert st["input_sorted"] == 0 and st["sorts"] == 2 and st["added"] == 2097 and st["input_distinct"] <= E


def test_edge_add_large_input_without_coalesce(ops, add_mirror, large):
    """k_ea_keys (the range check) and k_ea_copy over E rows."""
    src, dst, n, _ = large
    E = src.size
    assert rounds(E) == 2 and rounds(1 * E) == 2                                       # K = 1: k_ea_copy over K E rows
    got, _, st = add_both(ops, add_mirror, src, dst, n, w=add_cases.weights(E), ratio=[0.001], seed=add_cases.SEED, coalesce=False)
    assert st["sorts"] == 0 and got[0].shape[0] == E + 2097


def test_edge_add_many_added_rows(ops, add_mirror):
    """k_ea_draw, k_ea_heads_b and k_ea_runs_b over E added rows, and -- the 5,000 input rows are in no order -- k_ea_hash_probe over
    them too: lanes with one head to probe beside lanes with two."""
    E = cases.STRIDE_E
    src, dst, n = add_cases.distinct_rows(5000)
    ratio = (E + 0.5) / 5000
    assert int(5000 * ratio) == E and rounds(E) == 2 and rounds(E + 1) == 2
    got, _, st = add_both(ops, add_mirror, src, dst, n, ratio=ratio, seed=add_cases.SEED)
    assert st["input_sorted"] == 0 and st["sorts"] == 2 and st["added"] == E and tuple(got[2].shape) == (E, 2)
    assert 5000 < got[0].shape[0] <= 5000 + E
