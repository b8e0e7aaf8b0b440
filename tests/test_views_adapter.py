"""rLapViews.augmentors(): the siblings of one rLapViews share ONE library call per input (no GPU: the op is replaced by a stub
that counts its calls and labels every view with the call that made it)."""
import pytest
import torch

from rlap_amd import adapters, ops


@pytest.fixture
def calls(monkeypatch):
    log = []

    def fake_views(edge_index, edge_weights, num_nodes, num_remove, o_v, o_n, **kw):
        log.append((edge_index.data_ptr(), list(num_remove)))
        K = len(num_remove)
        call = len(log)
        # view k: one row [call, k, weight]: ids tell which call and which view a graph came from
        sc = torch.tensor([[float(call), float(k), 1.0] for k in range(K)], dtype=torch.float64)
        return sc, torch.arange(K + 1, dtype=torch.int64)

    monkeypatch.setattr(ops, "approximate_cholesky_views", fake_views)
    return log


def ids(g):
    return tuple(int(v) for v in g.edge_index[:, 0])   # (call, view)


def graph(n=10):
    a = torch.arange(n - 1)
    return torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])])


def test_one_call_per_step_for_the_pair(calls):
    x = torch.zeros(10, 2)
    ei = graph()
    aug1, aug2 = adapters.rLapViews(fracs=(0.2, 0.5)).augmentors()
    for step in range(3):
        g1 = aug1(x, ei)
        g2 = aug2(x, ei)
        assert ids(g1) == (step + 1, 0) and ids(g2) == (step + 1, 1)
    assert len(calls) == 3
    assert calls[0][1] == [int(0.2 * 10), int(0.5 * 10)]   # num_nodes = edge_index.max() + 1
    # either sibling may come first
    g2 = aug2(x, ei)
    g1 = aug1(x, ei)
    assert ids(g2) == (4, 1) and ids(g1) == (4, 0) and len(calls) == 4


def test_fresh_call_when_the_input_changes(calls):
    x = torch.zeros(10, 2)
    ei = graph()
    aug1, aug2 = adapters.rLapViews(fracs=(0.2, 0.5)).augmentors()
    aug1(x, ei)
    other = graph().clone()
    assert ids(aug2(x, other)) == (2, 1)          # another tensor: its own call, not the pending view of `ei`
    ei2 = graph()
    aug1(x, ei2)
    ei2[0, 0] = 1                                 # modified in place (version counter moves): the pending view is stale
    assert ids(aug2(x, ei2)) == (4, 1)
    assert len(calls) == 4


def test_no_view_is_handed_out_twice(calls):
    x = torch.zeros(10, 2)
    ei = graph()
    aug1, aug2 = adapters.rLapViews(fracs=(0.2, 0.5)).augmentors()
    assert ids(aug1(x, ei)) == (1, 0)
    assert ids(aug1(x, ei)) == (2, 0)             # called again before its sibling: a fresh call
    assert ids(aug2(x, ei)) == (2, 1)             # the sibling takes the view of the latest call
    assert ids(aug2(x, ei)) == (3, 1)             # ... once
    assert len(calls) == 3


def test_augment_returns_all_views_from_one_call(calls):
    x = torch.zeros(10, 2)
    gs = adapters.rLapViews(fracs=(0.1, 0.2, 0.3), keep_weights=True).augment((x, graph(), None))
    assert [ids(g) for g in gs] == [(1, 0), (1, 1), (1, 2)] and len(calls) == 1
    assert all(g.edge_weights is not None for g in gs)
