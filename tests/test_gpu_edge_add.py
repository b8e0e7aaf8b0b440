"""Edge adding on the device: ops.add_edges and the adapters on it, against the host mirror
(tests/csrc/edgeadd_mirror.cc around rlap_amd/csrc/rlap_edgeadd.h, the header the kernels include), whose rules
tests/test_edge_add_cpu.py ties to numpy and pure Python (tests/edge_add_cases.py).  The rules are integer arithmetic, one float64
multiply a draw and float64 additions in a stated order: rows, ptr, added and aptr are compared by equality of bits.  The shapes
are the smallest at which the kernels can go wrong: T = ROW_TILE merged positions a workgroup."""
import numpy as np
import pytest
import torch

import edge_add_cases as cases
import edgeadd_mirror

pytestmark = pytest.mark.gpu
T = cases.T


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return edgeadd_mirror.build(tmp_path_factory.mktemp("edgeadd"))


def on_device(src, dst):
    return torch.from_numpy(np.stack([src, dst])).cuda()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(got, want):
    """(rows, ptr, added, aptr) of the device against the mirror's dict, bit for bit."""
    ok = np.array_equal(bits(got[0].cpu().numpy()), bits(want["rows"])) and got[1].tolist() == want["ptr"].tolist()
    return ok and got[2].dtype == torch.int64 and np.array_equal(got[2].cpu().numpy(), want["added"]) and got[3].tolist() == want["aptr"].tolist()


def both(ops, mirror, src, dst, n, w=None, **kw):
    """The call on the device and by the mirror; asserts their equality and returns (device result, mirror result, last_stats)."""
    want = edgeadd_mirror.run(mirror, src, dst, n, w=w, **kw)
    got = ops.add_edges(on_device(src, dst), None if w is None else torch.from_numpy(w).cuda(), n, return_added=True, **kw)
    st = dict(ops.last_stats)
    assert same(got, want), (n, kw)
    assert st["rows_needed"] == got[0].shape[0] and st["added"] == got[2].shape[0]
    if kw.get("coalesce", True):
        assert st["input_sorted"] == want["input_sorted"] and st["input_distinct"] == want["input_distinct"]
    assert st["host_syncs"] == 1
    return got, want, st


def ratio_for(E, count):
    """A ratio with int(E * ratio) == count."""
    r = (count + 0.5) / E if count else 0.0
    assert int(E * r) == count
    return r


@pytest.mark.parametrize("name", list(cases.GRAPHS))
def test_against_the_mirror(ops, mirror, name):
    src, dst, n = cases.graph(name)
    for w in (None, cases.weights(src.size)):
        got, _, st = both(ops, mirror, src, dst, n, w=w, ratio=list(cases.RATIOS), seed=cases.SEED)
        assert st["input_sorted"] == 0 and st["sorts"] == 2 and st["launches"] > 0       # one sort of the input, one of both views' draws
        plain = ops.add_edges(on_device(src, dst), None if w is None else torch.from_numpy(w).cuda(), n, list(cases.RATIOS), cases.SEED)
        assert len(plain) == 2 and torch.equal(plain[0], got[0]) and torch.equal(plain[1], got[1])   # `added` changes no row
        again = ops.add_edges(on_device(src, dst), None if w is None else torch.from_numpy(w).cuda(), n, list(cases.RATIOS), cases.SEED, return_added=True)
        assert all(torch.equal(a, b) for a, b in zip(got, again))                        # two calls return equal bits


@pytest.mark.parametrize("n_a,num_add", cases.TILE_EDGE_PAIRS)
def test_merge_at_the_tile_edges(ops, mirror, n_a, num_add):
    """n_a distinct input pairs and num_add added rows (distinct too: the ids are wide), coalesced and not.  Without an input row the
    contract adds nothing, so for n_a = 0 the input is num_add copies of one row: n_a = 1."""
    if n_a == 0 and num_add > 0:
        src, dst, n = np.full(num_add, 5, dtype=np.int64), np.full(num_add, 3, dtype=np.int64), cases.WIDE_N
        ratio, n_a = 1.0, 1
    else:
        src, dst, n = cases.distinct_rows(n_a)
        ratio = ratio_for(n_a, num_add) if n_a else 0.0
    got, want, st = both(ops, mirror, src, dst, n, ratio=ratio, seed=cases.SEED)
    assert st["input_distinct"] == n_a and st["added"] == num_add and got[0].shape[0] == n_a + num_add   # no pair drawn twice at this width
    both(ops, mirror, src, dst, n, w=cases.weights(src.size), ratio=ratio, seed=cases.SEED, coalesce=False)
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["sorts"] == 0


def test_empty_lists(ops, mirror):
    empty = np.zeros(0, dtype=np.int64)
    got, _, st = both(ops, mirror, empty, empty, 5, ratio=[0.5, 2.5])                   # E = 0: empty views
    assert tuple(got[0].shape) == (0, 3) and got[1].tolist() == [0, 0, 0] and st["sorts"] == 0 and st["input_sorted"] == 1
    both(ops, mirror, empty, empty, 0, ratio=0.5)
    both(ops, mirror, empty, empty, 0, ratio=0.5, coalesce=False)
    src, dst, n = cases.graph("messy")
    w = cases.dyadic(src.size)
    got, _, st = both(ops, mirror, src, dst, n, w=w, ratio=0.0)                          # ratio = 0: the coalesced input alone
    keys, inv = np.unique(src * n + dst, return_inverse=True)
    sums = np.zeros(keys.size)
    np.add.at(sums, inv, w)
    assert st["added"] == 0 and st["sorts"] == 1 and np.array_equal(got[0].cpu().numpy(), np.stack([keys // n, keys % n, sums], 1))


def test_long_runs_of_equal_keys(ops, mirror):
    src, dst, _ = cases.graph("messy")
    got, _, st = both(ops, mirror, src % 2, dst % 2, 3, ratio=ratio_for(700, 3 * T + 7), seed=cases.SEED)   # N = 3: four possible pairs
    assert got[0].shape[0] == 4 and float(got[0][:, 2].sum()) == 700 + 3 * T + 7
    got, _, _ = both(ops, mirror, src % 2, dst % 2, 3, ratio=[ratio_for(700, 3 * T + 7), 0.5, ratio_for(700, T)], seed=cases.SEED)
    assert got[1].tolist() == [0, 4, 8, 12]
    got, _, _ = both(ops, mirror, src * 0, dst * 0, 2, ratio=ratio_for(700, 2 * T + 1))  # N = 2: every added row is (0, 0)
    assert got[0].tolist() == [[0.0, 0.0, 700.0 + 2 * T + 1]] and not bool(got[2].any())
    E = 2 * T + 5                                                                      # one run of 2T + 5 rows, general weights: input order
    w = cases.weights(E)
    for order in (np.arange(E), np.random.RandomState(1).permutation(E)):
        got, _, _ = both(ops, mirror, np.full(E, 3, dtype=np.int64), np.full(E, 1, dtype=np.int64), 9, w=w[order], ratio=0.0)
        s = 0.0
        for v in w[order].tolist():
            s += v
        assert got[0].tolist() == [[3.0, 1.0, s]]
    mixed = np.concatenate([np.full(E, 3, dtype=np.int64), src % 5])                   # the same run, scattered through unsorted rows
    perm = np.random.RandomState(2).permutation(mixed.size)
    both(ops, mirror, mixed[perm], np.concatenate([np.full(E, 1, dtype=np.int64), dst % 5])[perm], 9, w=cases.weights(mixed.size), ratio=0.3)


def test_ties_at_every_partition(ops, mirror):
    """The input holds exactly the pairs the view will draw (a first call's `added`): every key of B ties with a key of A, and every
    diagonal of the merge falls inside a tie."""
    E = 2 * T + 1
    src, dst, n = cases.distinct_rows(E, n=5000)
    first = ops.add_edges(on_device(src, dst), None, n, 1.0, cases.SEED, return_added=True)
    added = first[2].cpu().numpy()
    assert added.shape == (E, 2)
    got, _, st = both(ops, mirror, added[:, 0].copy(), added[:, 1].copy(), n, w=cases.weights(E), ratio=1.0, seed=cases.SEED)
    assert np.array_equal(got[2].cpu().numpy(), added)                                 # the same E and seed: the same draws
    assert got[0].shape[0] == st["input_distinct"] == np.unique(added[:, 0] * n + added[:, 1]).size
    cs, cd = cases.coalesced(added[:, 0], added[:, 1], n)                               # the same with a sorted input: n_a == n_b exactly
    m = cs.size
    got, _, st = both(ops, mirror, cs, cd, n, ratio=ratio_for(m, E), seed=cases.SEED)
    assert st["input_sorted"] == 1 and got[0].shape[0] == m and bool((got[0][:, 2] >= 2.0).all())


def test_one_sided_merges(ops, mirror):
    n = 2**20
    t = np.random.RandomState(8).permutation(T + 1).astype(np.int64)
    last = np.full(T + 1, n - 1, dtype=np.int64)                                       # the last node is never drawn: all of B before all of A
    got, _, _ = both(ops, mirror, last, t, n, ratio=1.0, seed=3)
    assert int(got[2][:, 0].max()) < n - 1 and bool((got[0][:T + 1, 2] == 1.0).all()) and bool((got[0][T + 1:, 0] == n - 1).all())
    got, _, _ = both(ops, mirror, np.zeros(T + 1, dtype=np.int64), t, n, ratio=1.0, seed=3)   # ... and the reverse: no draw has source 0
    assert int(got[2][:, 0].min()) > 0 and bool((got[0][:T + 1, 0] == 0).all())


def test_input_orders_give_identical_rows(ops, mirror):
    src, dst, n = cases.graph("messy")
    cs, cd = cases.coalesced(src, dst, n)
    w = cases.dyadic(cs.size)
    E = cs.size
    a, _, st_a = both(ops, mirror, cs, cd, n, w=w, ratio=[0.3, 0.4], seed=9)            # sorted and coalesced
    assert st_a["input_sorted"] == 1 and st_a["sorts"] == 1 and st_a["host_syncs"] == 1 and st_a["input_distinct"] == E
    order = np.lexsort((cs, cd))                                                       # (target, source) order, as the elimination emits
    b, _, st_b = both(ops, mirror, cs[order], cd[order], n, w=w[order], ratio=[0.3, 0.4], seed=9)
    assert st_b["input_sorted"] == 0 and st_b["sorts"] == 2
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # the same multiset with duplicates and loops, shuffled: each row split in two halves of its (dyadic) weight
    s2, d2, w2 = np.concatenate([cs, cs]), np.concatenate([cd, cd]), np.concatenate([w / 2, w / 2])
    perm = np.random.RandomState(4).permutation(2 * E)
    c = ops.add_edges(on_device(s2[perm], d2[perm]), torch.from_numpy(w2[perm]).cuda(), n, [ratio_for(2 * E, int(E * 0.3)), ratio_for(2 * E, int(E * 0.4))], 9)
    assert ops.last_stats["input_sorted"] == 0 and ops.last_stats["sorts"] == 2 and ops.last_stats["input_distinct"] == E
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and bool((cs == cd).any())
    sorted_dups = np.sort(perm % E)                                                    # ascending with duplicates: still no sort
    _, _, st = both(ops, mirror, cs[sorted_dups], cd[sorted_dups], n, w=w2[:2 * E][sorted_dups], ratio=0.3)
    assert st["input_sorted"] == 1 and st["sorts"] == 1 and st["input_distinct"] == E


@pytest.mark.parametrize("n", [2**10, 2**10 + 1, 2**16, 2**16 + 1])
def test_key_width_at_powers_of_two(ops, mirror, n):
    src, dst, _ = cases.distinct_rows(300, n=n, low=n - 40, high=n)                      # ids up to N - 1
    _, _, st = both(ops, mirror, src, dst, n, ratio=[0.5, 2.5, 1.0], seed=cases.SEED)
    assert st["sorts"] == 2                                                            # the one-sort path: the input, and all three views at once


def test_the_widest_keys_take_the_per_view_sorts(ops, mirror):
    n = 2**31 - 1
    src, dst, _ = cases.distinct_rows(300, n=n, low=n - 40, high=n)
    src[0], dst[1] = n - 1, n - 1                                                      # ids reach N - 1
    _, _, st = both(ops, mirror, src, dst, n, w=cases.weights(300), ratio=[0.5, 2.5, 1.0], seed=cases.SEED)
    assert st["sorts"] == 1 + 3                                                        # 62-bit keys: no room for the view number of K = 3
    _, _, st = both(ops, mirror, src, dst, n, ratio=[0.5, 0.0, 1.0], seed=cases.SEED)
    assert st["sorts"] == 1 + 2                                                        # a view without added rows sorts nothing
    _, _, st = both(ops, mirror, src, dst, n, ratio=[0.5, 2.5], seed=cases.SEED)
    assert st["sorts"] == 1 + 1                                                        # K = 2: one bit, which fits


def test_the_key_set_wraps_at_the_tables_end(ops, mirror):
    """Tiny inputs in no order whose key set (2 E slots, linear probing) has its occupied slots across the table's end: chosen with
    the model of tests/edge_add_cases.py, for which tests/test_edge_add_cpu.py shows that insertions wrap in every one of them and
    that among the added keys of these very calls probes cross the end both to their key and to an empty slot.  ptr and rows_needed
    come from the set, the rows from the sort that follows: a wrong wrap shows in the first two."""
    seeds = cases.wrapping_inputs()
    assert len(seeds) >= 20
    for seed in seeds:
        src, dst, n = cases.tiny_unsorted(seed)
        _, _, st = both(ops, mirror, src, dst, n, w=cases.weights(src.size), ratio=list(cases.WRAP_RATIOS), seed=cases.SEED)
        assert st["input_sorted"] == 0 and st["sorts"] == 2, seed


def test_views(ops, mirror):
    src, dst, n = cases.distinct_rows(T + 1, n=600)
    ei = on_device(src, dst)
    w = cases.weights(T + 1)
    dw = torch.from_numpy(w).cuda()
    for ratios in ([0.3], [0.3, 2.5], [0.3, 2.5, 0.0]):
        for coalesce in (True, False):
            many, _, _ = both(ops, mirror, src, dst, n, w=w, ratio=ratios, seed=40, coalesce=coalesce)
            p, q = many[1].tolist(), many[3].tolist()
            for k, r in enumerate(ratios):
                one = ops.add_edges(ei, dw, n, r, 40 + k, coalesce, return_added=True)
                assert torch.equal(one[0], many[0][p[k]:p[k + 1]]) and one[1].tolist() == [0, p[k + 1] - p[k]]
                assert torch.equal(one[2], many[2][q[k]:q[k + 1]]) and one[3].tolist() == [0, q[k + 1] - q[k]]
    ratios = [k / 16 for k in range(32)]                                               # K = 32 once
    _, _, st = both(ops, mirror, src, dst, n, ratio=ratios, seed=5)
    assert st["sorts"] == 2
    both(ops, mirror, src, dst, n, ratio=ratios, seed=5, coalesce=False)


def test_refusals(ops):
    src, dst, n = cases.graph("ba300")
    ei = on_device(src, dst)
    for coalesce in (True, False):
        with pytest.raises(ValueError, match="out of range"):
            ops.add_edges(ei, None, n - 1, coalesce=coalesce)
        bad = ei.clone()
        bad[1, 7] = -1
        with pytest.raises(ValueError):
            ops.add_edges(bad, None, n, coalesce=coalesce)
    for kw in (dict(ratio=[0.5] * 33), dict(ratio=-0.5), dict(ratio=float("nan")), dict(seed=1.5)):
        with pytest.raises(ValueError):
            ops.add_edges(ei, None, n, **kw)
    with pytest.raises(ValueError, match="num_nodes"):
        ops.add_edges(torch.zeros((2, 4), dtype=torch.int64, device="cuda"), None, None, 0.5)
    rows, ptr = ops.add_edges(ei, None, n, 0.5)                                         # the handle works after the refusals
    assert src.size < rows.shape[0] <= src.size + src.size // 2 and ptr.tolist() == [0, rows.shape[0]]


def test_downstream_plan_layer_and_elimination(ops, mirror):
    from rlap_amd import adapters
    src, dst, n = cases.graph("ba300")
    ei = on_device(src, dst)
    torch.manual_seed(0)
    x = torch.randn(n, 8, dtype=torch.float64, device="cuda")
    views = adapters.EdgeAddingViews((0.3, 0.4))
    plan = views.plan(adapters.Graph(x, ei, None))
    want = edgeadd_mirror.run(mirror, src, dst, n, ratio=[0.3, 0.4], seed=views.last_seed)   # the call's own seed
    ref = ops.edge_list_plan(torch.from_numpy(want["rows"]).cuda(), want["ptr"].tolist(), n)
    assert plan.layers == 2
    y = plan.propagate(x)
    assert tuple(y.shape) == (2, n, 8) and torch.equal(y, ref.propagate(x))
    conv = adapters.SnapshotGCNConv(8, 4).double().cuda()
    out = conv(x, plan)
    out.sum().backward()
    assert tuple(out.shape) == (2, n, 4) and conv.weight.grad is not None
    fixed = adapters.EdgeAddingViews((0.3, 0.4), views.last_seed)                       # an explicit seed repeats the views
    g1, g2 = (aug(x, ei, None) for aug in fixed.augmentors())
    p = want["ptr"].tolist()
    assert np.array_equal(g1.edge_index.cpu().numpy().T, want["rows"][:p[1], :2]) and np.array_equal(g2.edge_index.cpu().numpy().T, want["rows"][p[1]:, :2])
    assert g1.edge_weights is None
    one = adapters.EdgeAdding(0.3, views.last_seed)(x, ei, None)                        # max id + 1 nodes, as the reference: the same graph here
    assert torch.equal(one.edge_index, g1.edge_index)
    wg = adapters.EdgeAdding(0.3, 1)(x, ei, torch.full((src.size,), 0.5, dtype=torch.float64, device="cuda"))
    assert wg.edge_weights.shape[0] == wg.edge_index.shape[1] and set(wg.edge_weights.tolist()) <= {0.5, 1.0, 1.5, 2.0, 2.5}
    # an unweighted view, symmetrised here, through the elimination
    e = one.edge_index
    e = e[:, e[0] != e[1]]
    key = torch.unique(torch.cat([e[0] * n + e[1], e[1] * n + e[0]]))
    sym = torch.stack([key // n, key % n])
    sc = ops.approximate_cholesky(sym, None, n, n // 2, "degree", "asc")
    assert sc.shape[1] == 3 and sc.shape[0] > 0


def test_default_augmentors_give_independent_views(ops):
    from rlap_amd import adapters
    src, dst, n = cases.graph("ba300")
    ei = on_device(src, dst)
    aug1, aug2 = adapters.EdgeAdding(0.3), adapters.EdgeAdding(0.3)
    views = [aug1(None, ei).edge_index, aug2(None, ei).edge_index, aug1(None, ei).edge_index]
    assert all(v.shape[1] > src.size for v in views)
    assert not any(a.shape == b.shape and torch.equal(a, b) for i, a in enumerate(views) for b in views[i + 1:])
    pair = adapters.EdgeAddingViews((0.3, 0.3))
    g1, g2 = (aug(None, ei) for aug in pair.augmentors())
    assert not (g1.edge_index.shape == g2.edge_index.shape and torch.equal(g1.edge_index, g2.edge_index))


def test_one_host_synchronisation_whatever_the_order(ops):
    """One host synchronisation whether the keys ascend or not, and the sort of the input skipped when they do.  The host learns
    whether they ascend from the one read-back; for an input that is not sorted the row total in that read-back comes from a set of
    the input's keys, not from the sort, which follows with the rows in stream order ("One read-back")."""
    src, dst, n = cases.graph("messy")
    cs, cd = cases.coalesced(src, dst, n)
    ops.add_edges(on_device(cs, cd), None, n, [0.3, 0.4], 1)
    print("sorted input:", ops.last_stats)
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["sorts"] == 1
    ops.add_edges(on_device(src, dst), None, n, [0.3, 0.4], 1)
    print("shuffled input:", ops.last_stats)
    assert ops.last_stats["sorts"] == 2
    assert ops.last_stats["host_syncs"] == 1
