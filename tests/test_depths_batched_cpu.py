"""approximate_cholesky_depths with node_ptr / views, and rLapDepths(views=R), without a GPU: the argument checks run before any
device or library call, and the adapter makes one call and hands out R runs of K graphs (the op is replaced by a stub)."""
import pytest
import torch

from rlap_amd import _lib, adapters, ops


def graph(n=10):
    a = torch.arange(n - 1)
    return torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])])


@pytest.fixture
def no_device(monkeypatch):
    def reached(*a, **k):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    monkeypatch.setattr(_lib, "load", reached)


@pytest.mark.parametrize("num_remove,node_ptr,views", [
    ([[[1, 2, 3]], [[0, 5, 3]]], [0, 4, 8, 10], 1),          # column (0, 0) decreases
    ([[[1, 2]], [[1, 3]]], [0, 4, 8, 10], 1),                # (D, K, G) with G = 2 for a batch of 3 graphs
    ([[[1, 2, 3]]], [0, 4, 8, 10], 2),                       # K = 1 for views = 2
    ([[1, 2, 3], [2, 3, 4]], [0, 4, 8, 10], 1),              # 2-D: neither (D,) nor (D, K, G)
    ([2, 1], [0, 4, 8, 10], 1),                              # a decreasing 1-D list
    ([1, 2], [0, 4, 8, 11], 1),                              # node_ptr[-1] != num_nodes
    ([1, 2], [0, 4, 3, 10], 1),                              # node_ptr decreases
    ([1, 2], [1, 4, 10], 1),                                 # node_ptr[0] != 0
    ([1.0, 2.0], [0, 4, 8, 10], 1),                          # not integers
    ([1, 2.5], None, 2),
    ([True, 3], None, 2),
    (torch.tensor([[[1.0]], [[2.0]]]), [0, 10], 1),
    ([[[1]], [["2"]]], [0, 10], 1),
    ([], [0, 10], 1),
    ([1, 2], None, 0),                                       # views < 1
    ([1, 2], None, 1.5),
    ([1, 2], [0.0, 10.0], 1),
])
def test_bad_arguments_raise_value_error_before_the_device(no_device, num_remove, node_ptr, views):
    with pytest.raises(ValueError):
        ops.approximate_cholesky_depths(graph(), None, 10, num_remove, "random", "asc", node_ptr=node_ptr, views=views)


def test_the_depth_table_layout():
    np_, t, K, G = ops._depths_table([1, 4], 10, [0, 4, 10], 3)
    assert np_.tolist() == [0, 4, 10] and (K, G) == (3, 2) and t.tolist() == [[1] * 6, [4] * 6]
    cols = torch.arange(2 * 3 * 2).reshape(2, 3, 2)   # t[d][k][g] = 6 d + 2 k + g: row d, column k * G + g
    _, t, _, _ = ops._depths_table(cols, 10, [0, 4, 10], 3)
    assert t.tolist() == [list(range(6)), list(range(6, 12))] and t.dtype == torch.int64
    _, t, K, G = ops._depths_table((0, 0, 7), 5, None, 1)   # zero and equal neighbours are fine
    assert (K, G) == (1, 1) and t.tolist() == [[0], [0], [7]]


def test_one_graph_lists_keep_the_single_graph_path(monkeypatch):
    seen = []
    monkeypatch.setattr(ops, "_depths_views", lambda *a: seen.append("views") or (None, None))
    monkeypatch.setattr(ops, "_depths_list", lambda nr: seen.append("list") or (_ for _ in ()).throw(ValueError("stop")))
    with pytest.raises(ValueError):
        ops.approximate_cholesky_depths(graph(), None, 10, [1, 2], "random", "asc")
    ops.approximate_cholesky_depths(graph(), None, 10, [1, 2], "random", "asc", views=2)
    ops.approximate_cholesky_depths(graph(), None, 10, [1, 2], "random", "asc", node_ptr=[0, 10])
    ops.approximate_cholesky_depths(graph(), None, 10, [[[1]], [[2]]], "random", "asc")
    assert seen == ["list", "views", "views", "views"]


@pytest.fixture
def calls(monkeypatch):
    log = []

    def fake_depths(edge_index, edge_weights, num_nodes, num_remove, o_v, o_n, **kw):
        log.append((num_nodes, list(num_remove), o_v, o_n, kw))
        D, R = len(num_remove), kw.get("views", 1)
        # snapshot (d, r), rows depth-major then view: one row [d, r, weight]
        sc = torch.tensor([[float(d), float(r), 1.0] for d in range(D) for r in range(R)], dtype=torch.float64)
        return sc, torch.arange(D * R + 1, dtype=torch.int64)

    monkeypatch.setattr(ops, "approximate_cholesky_depths", fake_depths)
    return log


def test_adapter_views_makes_one_call_and_returns_runs(calls):
    x = torch.zeros(10, 2)
    ei = graph(37)
    fracs = (0.1, 0.25, 0.5)
    runs = adapters.rLapDepths(fracs=fracs, seed=5, keep_weights=True, views=4).augment((x, ei, None))
    assert len(calls) == 1
    n, ts, o_v, o_n, kw = calls[0]
    assert n == 37 and ts == [int(f * 37) for f in fracs] and kw["views"] == 4 and kw["seed"] == 5
    assert len(runs) == 4 and all(len(r) == len(fracs) for r in runs)
    assert [[tuple(int(v) for v in g.edge_index[:, 0]) for g in r] for r in runs] == [[(d, r) for d in range(3)] for r in range(4)]
    assert all(g.edge_weights is not None and g.x is x for r in runs for g in r)
    flat = adapters.rLapDepths(fracs=fracs)(x, ei)   # views=None: today's flat list, no `views` argument
    assert len(calls) == 2 and "views" not in calls[1][4] and len(flat) == 3
