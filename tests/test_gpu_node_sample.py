"""Node dropping and random-walk subgraph views on the device: ops.sample_subgraphs and the adapters on it, against
the host mirror (tests/csrc/nodesample_mirror.cc around rlap_amd/csrc/rlap_nodesample.h, the header the kernels include), whose
rules tests/test_node_sample_cpu.py ties to numpy and pure Python on the very inputs used here (tests/node_sample_cases.py).
The rules are integer arithmetic and one float64 multiply: node sets, walks, rows and ptr are compared by equality."""
import numpy as np
import pytest
import torch

import node_sample_cases as cases
import nodesample_mirror

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return nodesample_mirror.build(tmp_path_factory.mktemp("nodesample"))


def on_device(src, dst):
    return torch.from_numpy(np.stack([src, dst])).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(got, want):
    """(rows, ptr, nodes[, walks]) of the device against the mirror's dict, bit for bit."""
    ok = np.array_equal(bits(got[0].cpu().numpy()), bits(want["rows"])) and got[1].tolist() == want["ptr"].tolist()
    ok = ok and got[2].dtype == torch.bool and np.array_equal(got[2].cpu().numpy(), want["nodes"])
    if len(got) > 3:
        ok = ok and got[3].dtype == torch.int64 and np.array_equal(got[3].cpu().numpy(), want["walks"])
    return ok


@pytest.mark.parametrize("name", list(cases.GRAPHS))
def test_against_the_mirror(ops, mirror, name):
    src, dst, n = cases.graph(name)
    ei, w = on_device(src, dst), cases.weights(src.size)
    dw = torch.from_numpy(w).cuda()
    want = nodesample_mirror.run(mirror, src, dst, n, w=w, p=cases.PS, seed=cases.SEED)
    got = ops.sample_subgraphs(ei, dw, n, "drop", list(cases.PS), seed=cases.SEED, return_nodes=True)
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["rows_needed"] == got[0].shape[0]
    assert same(got, want) and (name != "ba300" or 0 < got[0].shape[0] < 2 * src.size)   # the weights reach column 2 untouched
    plain = ops.sample_subgraphs(ei, dw, n, "drop", list(cases.PS), seed=cases.SEED)
    assert len(plain) == 2 and torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])   # the node mask changes no row
    for L in cases.WALK_LENGTHS:                                                  # the hub of 513, the sink and the loop rows: "directed"
        kw = dict(scheme="walk", num_seeds=[n // 3, n // 5 + 1], walk_length=L, seed=cases.SEED)
        want = nodesample_mirror.run(mirror, src, dst, n, w=w, **kw)
        got = ops.sample_subgraphs(ei, dw, n, return_nodes=True, return_walks=True, **kw)
        assert ops.last_stats["host_syncs"] == 1 and same(got, want), (name, L)
        plain = ops.sample_subgraphs(ei, dw, n, **kw)                               # the walks are written only when asked for
        assert len(plain) == 2 and torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])


@pytest.mark.parametrize("E", cases.TILE_EDGE_ROWS)
def test_compaction_at_the_tile_edges(ops, mirror, E):
    src, dst, n = cases.random_rows(E)
    ei = on_device(src, dst)
    for K in (1, 2, 3):
        want = nodesample_mirror.run(mirror, src, dst, n, p=[0.3] * K, seed=cases.SEED)
        assert same(ops.sample_subgraphs(ei, None, n, "drop", [0.3] * K, seed=cases.SEED, return_nodes=True), want)
        kw = dict(scheme="walk", num_seeds=[40] * K, walk_length=3, seed=cases.SEED)
        want = nodesample_mirror.run(mirror, src, dst, n, **kw)
        assert same(ops.sample_subgraphs(ei, None, n, return_nodes=True, return_walks=True, **kw), want)
    if E == cases.ROW_TILE + 1:                                                     # K = 32 once
        ps = [k / 40 for k in range(32)]
        assert same(ops.sample_subgraphs(ei, None, n, "drop", ps, seed=5, return_nodes=True), nodesample_mirror.run(mirror, src, dst, n, p=ps, seed=5))
        kw = dict(scheme="walk", num_seeds=list(range(32)), walk_length=2, seed=5)
        assert same(ops.sample_subgraphs(ei, None, n, return_nodes=True, return_walks=True, **kw), nodesample_mirror.run(mirror, src, dst, n, **kw))


@pytest.mark.parametrize("n", cases.WORD_EDGE_NODES)
def test_bitmap_word_edges(ops, mirror, n):
    src, dst, _ = cases.random_rows(300, n)
    ei = on_device(src, dst)
    for p in (0.0, 0.5, 1.0):
        assert same(ops.sample_subgraphs(ei, None, n, "drop", [p, 0.25], seed=1, return_nodes=True), nodesample_mirror.run(mirror, src, dst, n, p=[p, 0.25], seed=1))
    kw = dict(scheme="walk", num_seeds=[n // 2 + 1, 3], walk_length=4, seed=1)
    assert same(ops.sample_subgraphs(ei, None, n, return_nodes=True, return_walks=True, **kw), nodesample_mirror.run(mirror, src, dst, n, **kw))


@pytest.mark.parametrize("n", cases.TOP_ID_NODES)
def test_walks_through_the_top_id(ops, mirror, n):
    """Id n - 1 -- bit 0 of the bitmap's last word, a word of its own -- as a walk's start, as a row's target and as a row's source:
    the mirror's walks start on it, arrive at it and leave it (the WORD_EDGE_NODES cases reach it only by chance)."""
    src, dst, _ = cases.top_id_rows(n)
    kw = cases.top_id_walk(n)
    want = nodesample_mirror.run(mirror, src, dst, n, **kw)
    assert cases.passes_through(want["walks"], n - 1) == (True, True, True) and want["nodes"][0, n - 1]
    got = ops.sample_subgraphs(on_device(src, dst), None, n, return_nodes=True, return_walks=True, **kw)
    assert ops.last_stats["host_syncs"] == 1 and same(got, want)
    assert bool(got[2][0, n - 1]) and (got[0][:, :2] == n - 1).any()               # the top id is in the set and in the rows kept


@pytest.mark.parametrize("walkers", cases.WALKER_COUNTS)
def test_walker_counts_across_wave_and_workgroup_edges(ops, mirror, walkers):
    src, dst, n = cases.graph("directed")
    ei = on_device(src, dst)
    kw = dict(scheme="walk", num_seeds=[walkers, 65, walkers], walk_length=10, seed=cases.SEED)
    want = nodesample_mirror.run(mirror, src, dst, n, **kw)
    got = ops.sample_subgraphs(ei, None, n, return_nodes=True, return_walks=True, **kw)
    assert tuple(got[3].shape) == (2 * walkers + 65, 11) and same(got, want)
    if walkers == 0:
        assert got[1][0] == got[1][1] and got[1][2] == got[1][3] and not got[2][0].any()      # empty views: equal offsets


def test_the_hub_the_sink_and_the_loop_rows(ops, mirror):
    """Enough walkers on the hand-made list that the hub's 513 outgoing rows, the sink and the loop rows are all walked."""
    src, dst, n = cases.graph("directed")
    kw = dict(scheme="walk", num_seeds=[20000], walk_length=10, seed=cases.SEED)
    want = nodesample_mirror.run(mirror, src, dst, n, **kw)
    w = want["walks"]
    after_hub = w[:, 1:][w[:, :-1] == 6]
    assert after_hub.size > 50 and np.unique(after_hub).size > 40                      # many of the hub's rows are followed
    assert ((w[:, :-1] == 9) & (w[:, 1:] == 9)).any() and (w[:, :-1] == 7).any()        # the sink and the id without rows keep their walkers
    assert ((w[:, :-1] == 3) & (w[:, 1:] == 3)).any() and ((w[:, :-1] == 5) & (w[:, 1:] == 5)).any()   # loop rows are followed
    assert same(ops.sample_subgraphs(on_device(src, dst), None, n, return_nodes=True, return_walks=True, **kw), want)


def test_views_repeats_weights_and_empty_views(ops, mirror):
    src, dst, n = cases.graph("ba300")
    ei, E = on_device(src, dst), src.size
    w = torch.from_numpy(cases.weights(E)).cuda()
    for kw, per_view in ((dict(scheme="drop", p=[0.2, 0.5, 0.35]), "p"), (dict(scheme="walk", num_seeds=[30, 0, 90], walk_length=4), "num_seeds")):
        many = ops.sample_subgraphs(ei, w, n, seed=40, return_nodes=True, return_walks=per_view == "num_seeds", **kw)
        again = ops.sample_subgraphs(ei, w, n, seed=40, return_nodes=True, return_walks=per_view == "num_seeds", **kw)
        assert all(torch.equal(a, b) for a, b in zip(many, again))                  # a repeated call returns equal bits
        p, first = many[1].tolist(), 0
        for k, value in enumerate(kw[per_view]):
            one = ops.sample_subgraphs(ei, w, n, seed=40 + k, return_nodes=True, return_walks=per_view == "num_seeds", **dict(kw, **{per_view: value}))
            assert torch.equal(one[0], many[0][p[k]:p[k + 1]]) and one[1].tolist() == [0, p[k + 1] - p[k]] and torch.equal(one[2][0], many[2][k])
            if per_view == "num_seeds":
                assert torch.equal(one[3], many[3][first:first + value])
                first += value
        m = many[2][0][ei[0]] & many[2][0][ei[1]]                                   # both ends in the set; edge_weight reaches column 2
        assert 0 < p[1] < E and torch.equal(many[0][:p[1]], torch.stack([ei[0][m].double(), ei[1][m].double(), w[m]], 1))
    rows, ptr, nodes = ops.sample_subgraphs(ei, None, n, "drop", [1.0, 0.0, 1.0], return_nodes=True)
    assert ptr.tolist() == [0, 0, E, E] and not nodes[0].any() and nodes[1].all() and torch.equal(rows[:, :2].long().t(), ei)   # empty views
    assert bool((rows[:, 2] == 1.0).all())
    none = torch.zeros((2, 0), dtype=torch.int64, device="cuda")
    rows, ptr, nodes, walks = ops.sample_subgraphs(none, None, 5, "walk", num_seeds=[9, 2], walk_length=6, return_nodes=True, return_walks=True)
    assert tuple(rows.shape) == (0, 3) and ptr.tolist() == [0, 0, 0] and bool((walks == walks[:, :1]).all()) and nodes.any()   # E = 0: walkers stay
    rows, ptr, nodes = ops.sample_subgraphs(none, None, 0, "drop", [0.5], return_nodes=True)
    assert tuple(rows.shape) == (0, 3) and ptr.tolist() == [0, 0] and tuple(nodes.shape) == (1, 0)


def test_a_batch_never_walks_across_graphs(ops):
    src, dst, n = cases.graph("two_ba50")
    walks = ops.sample_subgraphs(on_device(src, dst), None, n, "walk", num_seeds=400, walk_length=10, seed=cases.SEED, return_walks=True)[2]
    side = walks >= 50
    assert bool((side == side[:, :1]).all()) and bool(side[:, 0].any()) and not bool(side[:, 0].all())


def test_refusals(ops):
    src, dst, n = cases.graph("ba300")
    ei = on_device(src, dst)
    for kw in (dict(scheme="drop", p=0.5), dict(scheme="walk", num_seeds=10)):
        with pytest.raises(ValueError, match="out of range"):
            ops.sample_subgraphs(ei, None, n - 1, **kw)
        bad = ei.clone()
        bad[1, 7] = -1
        with pytest.raises(ValueError):
            ops.sample_subgraphs(bad, None, n, **kw)
    for kw in (dict(p=[0.5] * 33), dict(p=1.5), dict(scheme="katz"), dict(scheme="walk"), dict(scheme="walk", num_seeds=3, walk_length=1025)):
        with pytest.raises(ValueError):
            ops.sample_subgraphs(ei, None, n, **kw)
    rows, ptr = ops.sample_subgraphs(ei, None, n, "walk", num_seeds=50)              # the handle works after the refusals
    assert 0 < rows.shape[0] < src.size and ptr.tolist() == [0, rows.shape[0]]


def test_plan_of_the_views_through_the_layer(ops):
    from rlap_amd import adapters
    src, dst, n = cases.graph("ba300")
    ei = on_device(src, dst)
    torch.manual_seed(0)
    x = torch.randn(n, 8, dtype=torch.float64, device="cuda")
    views = adapters.NodeSampleViews("walk", (90, 120), 10)
    plan = views.plan(adapters.Graph(x, ei, None))
    _, _, nodes = ops.sample_subgraphs(ei, None, n, "walk", num_seeds=[90, 120], walk_length=10, seed=views.last_seed, return_nodes=True)   # the call's own seed
    kept = [ei[:, nodes[k][ei[0]] & nodes[k][ei[1]]] for k in range(2)]             # the rows filtered in torch with the returned node sets
    rows = torch.cat([torch.stack([e[0].double(), e[1].double(), torch.ones(e.shape[1], dtype=torch.float64, device="cuda")], 1) for e in kept])
    ref = ops.edge_list_plan(rows, [0, kept[0].shape[1], kept[0].shape[1] + kept[1].shape[1]], n)
    assert plan.layers == 2 and 0 < kept[0].shape[1] < src.size
    conv = adapters.SnapshotGCNConv(8, 4).double().cuda()
    out = conv(x, plan)
    assert tuple(out.shape) == (2, n, 4) and torch.equal(out, conv(x, ref))
    out.sum().backward()
    assert conv.weight.grad is not None and bool(conv.weight.grad.abs().sum() > 0)
    fixed = adapters.NodeSampleViews("walk", (90, 120), 10, views.last_seed)          # an explicit seed repeats the views
    g1, g2 = (aug(x, ei, None) for aug in fixed.augmentors())
    assert torch.equal(g1.edge_index, kept[0]) and torch.equal(g2.edge_index, kept[1]) and g1.edge_weights is None
    one = adapters.RWSampling(90, 10, views.last_seed)(x, ei, None)                   # max id + 1 nodes, as PyGCL: the same graph here
    assert torch.equal(one.edge_index, kept[0])


def test_default_augmentors_give_independent_views(ops):
    """The reference's (aug1, aug2) are built with the same arguments and called at every step: without an explicit seed neither the
    two augmentors nor two calls of one return the same view."""
    from rlap_amd import adapters
    src, dst, n = cases.graph("ba300")
    ei, E = on_device(src, dst), src.size
    for make in (lambda: adapters.NodeDropping(0.3), lambda: adapters.RWSampling(60, 10)):
        aug1, aug2 = make(), make()
        views = [aug1(None, ei).edge_index, aug2(None, ei).edge_index, aug1(None, ei).edge_index]
        assert all(0 < v.shape[1] < E for v in views)
        assert not any(a.shape == b.shape and torch.equal(a, b) for i, a in enumerate(views) for b in views[i + 1:])
    for pair in (adapters.NodeSampleViews("drop", (0.3, 0.3)), adapters.NodeSampleViews("walk", (60, 60))):
        g1, g2 = (aug(None, ei) for aug in pair.augmentors())
        h1, _ = (aug(None, ei) for aug in pair.augmentors())
        assert not (g1.edge_index.shape == g2.edge_index.shape and torch.equal(g1.edge_index, g2.edge_index))
        assert not (g1.edge_index.shape == h1.edge_index.shape and torch.equal(g1.edge_index, h1.edge_index))
