"""approximate_cholesky_depths / rLapDepths without a GPU: the argument checks run before any device or library call, and the
adapter derives its depths from `fracs` the way rLap does (the op is replaced by a stub that records what it was asked)."""
import numpy as np
import pytest
import torch

from rlap_amd import adapters, ops


def graph(n=10):
    a = torch.arange(n - 1)
    return torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])])


@pytest.mark.parametrize("bad", [[], [5, 3], [1, 4, 2], [1.0, 2.0], [1, 2.5], [True, 3], ["3"], 7, torch.tensor([1.0, 2.0]),
                                 torch.tensor([3, 1])])
def test_bad_depth_lists_raise_value_error_before_the_device(bad, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(ops, "_device_for", no_device)
    monkeypatch.setattr(ops, "_handle_obj", no_device)
    with pytest.raises(ValueError):
        ops.approximate_cholesky_depths(graph(), None, 10, bad, "random", "asc")


def test_good_depth_lists_are_accepted():
    assert ops._depths_list([0, 0, 3, 3, 12]) == [0, 0, 3, 3, 12]
    assert ops._depths_list((np.int64(2), 5)) == [2, 5]
    assert ops._depths_list(torch.tensor([1, 4])) == [1, 4]


@pytest.fixture
def calls(monkeypatch):
    log = []

    def fake_depths(edge_index, edge_weights, num_nodes, num_remove, o_v, o_n, **kw):
        log.append((num_nodes, list(num_remove), o_v, o_n, kw))
        K = len(num_remove)
        # snapshot k: one row [k, t_k, weight]
        sc = torch.tensor([[float(k), float(t), 1.0] for k, t in enumerate(num_remove)], dtype=torch.float64)
        return sc, torch.arange(K + 1, dtype=torch.int64)

    monkeypatch.setattr(ops, "approximate_cholesky_depths", fake_depths)
    return log


def test_depths_from_fracs_like_rlap(calls):
    x = torch.zeros(10, 2)
    ei = graph(37)   # num_nodes = edge_index.max() + 1 = 37
    fracs = (0.1, 0.25, 0.5)
    aug = adapters.rLapDepths(fracs=fracs, o_v="degree", o_n="random", seed=5, keep_weights=True)
    gs = aug.augment((x, ei, None))
    assert len(calls) == 1
    n, ts, o_v, o_n, kw = calls[0]
    assert n == 37 and ts == [int(f * 37) for f in fracs] == aug.num_remove
    assert (o_v, o_n, kw["seed"], kw["mode"]) == ("degree", "random", 5, "exact")
    assert [tuple(int(v) for v in g.edge_index[:, 0]) for g in gs] == [(k, int(f * 37)) for k, f in enumerate(fracs)]
    assert all(g.edge_weights is not None and g.x is x for g in gs)
    g = adapters.rLapDepths()(x, ei)   # PyGCL-style call: (x, edge_index, edge_weight)
    assert len(g) == 3 and calls[1][1] == [int(f * 37) for f in (0.1, 0.2, 0.3)] and g[0].edge_weights is None
