"""Snapshot statistics on the device (ops.snapshot_stats, rlap_snapshot_stats): node counts against torch.unique, row counts
against ptr, and the largest adjacency eigenvalue against a dense float64 eigvalsh (small snapshots) or a Lanczos with full
reorthogonalisation in torch (a BA(200k, 5) snapshot); edge cases, determinism, and that the call leaves its inputs and later
calls untouched."""
import numpy as np
import pytest
import torch

from util import ba_graph, grid2d, path, star, sym_weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def check_counts(ops, sc, ptr, num_nodes, node_ptr=None):
    st = ops.snapshot_stats(sc, ptr, num_nodes, node_ptr=node_ptr)
    p = torch.as_tensor(ptr).cpu()
    S = p.numel() - 1
    nodes = st["nodes"].cpu()
    rows = st["rows"].cpu()
    for s in range(S):
        part = sc[int(p[s]):int(p[s + 1]), :2]
        assert int(nodes[s]) == torch.unique(part).numel(), s
        assert int(rows[s]) == int(p[s + 1] - p[s]), s
    assert bool(st["converged"].all())
    return st


def dense_lambda(sc, n, weighted):
    A = torch.zeros((n, n), dtype=torch.float64, device=sc.device)
    r, c = sc[:, 0].long(), sc[:, 1].long()
    A.index_put_((r, c), sc[:, 2] if weighted else torch.ones_like(sc[:, 2]), accumulate=True)
    assert torch.allclose(A, A.t(), rtol=1e-12, atol=0)
    return float(torch.linalg.eigvalsh(0.5 * (A + A.t()))[-1]) if sc.shape[0] else 0.0


def cuda_ei(ei):
    return torch.from_numpy(np.ascontiguousarray(ei)).cuda()


@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_counts_single(ops, o_v):
    n = 3000
    ei = cuda_ei(ba_graph(n, 6, 3))
    sc = ops.approximate_cholesky(ei, None, n, n // 2, o_v, "asc", seed=5, return_device="same")
    st = check_counts(ops, sc, [0, sc.shape[0]], n)
    assert int(st["nodes"][0]) <= n - n // 2


def test_counts_batch_views_depths(ops):
    gs = [ba_graph(500, 4, 1), grid2d(20, 30), ba_graph(800, 3, 2)]
    ns = [500, 600, 800]
    node_ptr = np.concatenate([[0], np.cumsum(ns)])
    N = int(node_ptr[-1])
    ei = cuda_ei(np.concatenate([e + node_ptr[g] for g, e in enumerate(gs)], axis=1))
    sc, ptr = ops.approximate_cholesky_batched(ei, None, node_ptr, [250, 100, 700], "random", "asc", seed=3)
    check_counts(ops, sc, ptr, N, node_ptr=node_ptr)
    sc, ptr = ops.approximate_cholesky_views(ei, None, N, [[100, 200, 300], [400, 500, 790]], "degree", "asc", node_ptr=node_ptr, seed=4)
    check_counts(ops, sc, ptr, N, node_ptr=node_ptr)
    t = [[[10, 20, 30], [40, 50, 60]], [[200, 300, 400], [250, 350, 450]], [[499, 599, 799], [300, 400, 500]]]
    sc, ptr = ops.approximate_cholesky_depths(ei, None, N, t, "random", "asc", node_ptr=node_ptr, views=2, seed=6)
    st = check_counts(ops, sc, ptr, N, node_ptr=node_ptr)
    assert int(st["nodes"][2 * 6 + 0]) == 0 and float(st["lambda_max"][2 * 6 + 0]) == 0.0   # (graph 0 at depth 499 = n - 1)
    # a single graph's views (node_ptr None: every id range is [0, N))
    e = cuda_ei(gs[0])
    sc, ptr = ops.approximate_cholesky_views(e, None, 500, [100, 250, 400], "random", "asc", seed=8)
    check_counts(ops, sc, ptr, 500)


GRAPHS = {
    "ba": lambda: (ba_graph(3000, 5, 7), 3000),
    "ba_dense": lambda: (ba_graph(2000, 12, 8), 2000),
    "grid": lambda: (grid2d(40, 50), 2000),
    "star": lambda: (star(2500), 2500),
    "path": lambda: (path(1500), 1500),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("weighted", [False, True])
def test_lambda_small_against_eigvalsh(ops, name, weighted):
    ei_np, n = GRAPHS[name]()
    w = torch.from_numpy(sym_weights(ei_np, n, 9)).cuda() if weighted else None
    ei = cuda_ei(ei_np)
    t = [0, n // 10, n // 4, n // 2]
    sc, ptr = ops.approximate_cholesky_depths(ei, w, n, t, "random", "asc", seed=11)
    st = ops.snapshot_stats(sc, ptr, n, weighted=weighted)
    assert bool(st["converged"].all())
    for k in range(len(t)):
        part = sc[int(ptr[k]):int(ptr[k + 1])]
        ref = dense_lambda(part, n, weighted)
        got = float(st["lambda_max"][k])
        assert abs(got - ref) <= 1e-9 * abs(ref), (k, got, ref)


def _graph_sc(edges, n):
    """(m, 3) rows of an unweighted symmetric graph grouped by column, as the output pass lays them out."""
    ei = torch.as_tensor(edges, dtype=torch.int64)
    order = torch.argsort(ei[1] * n + ei[0])
    ei = ei[:, order]
    return torch.stack([ei[0].double(), ei[1].double(), torch.ones(ei.shape[1], dtype=torch.float64)], 1).cuda()


def test_bipartite_disconnected_and_k2(ops):
    # path and grid: bipartite (lambda_min = -lambda_max); two components of different lambda; K2
    p50 = path(50)
    g = grid2d(7, 9)
    two = np.concatenate([star(6), ba_graph(40, 3, 2) + 6], axis=1)   # star K_{1,5} (sqrt 5) and a BA graph (larger)
    k2 = np.array([[0, 1], [1, 0]])
    cases = [(p50, 50, 2 * np.cos(np.pi / 51)), (g, 63, 2 * np.cos(np.pi / 8) + 2 * np.cos(np.pi / 10)), (two, 46, None), (k2, 2, 1.0)]
    scs, ptr = [], [0]
    for e, n, _ in cases:
        scs.append(_graph_sc(e, 64))
        ptr.append(ptr[-1] + scs[-1].shape[0])
    sc = torch.cat(scs)
    st = ops.snapshot_stats(sc, ptr, 64)
    assert bool(st["converged"].all())
    for s, (e, n, exact) in enumerate(cases):
        ref = dense_lambda(scs[s], 64, False) if exact is None else exact
        assert abs(float(st["lambda_max"][s]) - ref) <= 1e-9 * ref, (s, float(st["lambda_max"][s]), ref)
        assert int(st["nodes"][s]) == n
    lam_star = np.sqrt(5.0)
    assert float(st["lambda_max"][2]) > lam_star + 1.0   # (the larger component wins, not the first one met)


def test_empty_snapshot(ops):
    n = 200
    ei = cuda_ei(ba_graph(n, 3, 1))
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, [n - 1, n + 5], "degree", "asc")
    assert int(ptr[-1]) == 0
    st = ops.snapshot_stats(sc, ptr, n)
    for key in ("nodes", "rows", "lambda_max", "iters"):
        assert st[key].cpu().tolist() == [0, 0], key
    st = ops.snapshot_stats(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), [0, 0, 0], n)
    assert st["lambda_max"].cpu().tolist() == [0.0, 0.0]


def lanczos_reference(sc, n, steps):
    """Largest eigenvalue by Lanczos with full reorthogonalisation (torch float64, sparse A) from the normalised ones vector on
    the non-isolated ids."""
    r, c = sc[:, 0].long(), sc[:, 1].long()
    A = torch.sparse_coo_tensor(torch.stack([r, c]), torch.ones_like(sc[:, 2]), (n, n)).coalesce().to_sparse_csr()
    ids = torch.unique(c)
    q = torch.zeros(n, dtype=torch.float64, device=sc.device)
    q[ids] = 1.0 / np.sqrt(ids.numel())
    V = [q]
    al, be = [], []
    for j in range(steps):
        w = A @ V[-1]
        al.append(float(w @ V[-1]))
        Vm = torch.stack(V, 1)
        w = w - Vm @ (Vm.t() @ w)
        w = w - Vm @ (Vm.t() @ w)
        b = float(torch.linalg.norm(w))
        be.append(b)
        V.append(w / b)
    T = np.diag(al) + np.diag(be[:-1], 1) + np.diag(be[:-1], -1)
    return float(np.linalg.eigvalsh(T)[-1])


def test_large_snapshot_against_full_reorthogonalisation(ops):
    from rlap_amd import graphs
    n = 200000
    ei = graphs.barabasi_albert(n, 5, 1).cuda()
    sc = ops.approximate_cholesky(ei, None, n, n // 2, "random", "asc", seed=2, return_device="same")
    st = ops.snapshot_stats(sc, [0, sc.shape[0]], n)
    assert ops.last_stats["large_segments"] == 1
    assert bool(st["converged"][0])
    assert int(st["nodes"][0]) == torch.unique(sc[:, :2]).numel()
    ref = lanczos_reference(sc, n, 150)
    got = float(st["lambda_max"][0])
    assert abs(got - ref) <= 1e-9 * ref, (got, ref)


def test_deterministic_and_isolated(ops):
    n = 20000
    ei = cuda_ei(ba_graph(n, 4, 5))
    t = [n // 8, n // 4, n // 2]
    args = (ei, None, n, t, "random", "asc")
    before, _ = ops.approximate_cholesky_depths(*args, seed=9)
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, t, "random", "asc", seed=3, views=2)
    sc0, ptr0 = sc.clone(), ptr.clone()
    a = ops.snapshot_stats(sc, ptr, n, weighted=True)
    b = ops.snapshot_stats(sc, ptr, n, weighted=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(sc, sc0) and torch.equal(ptr, ptr0)
    after, _ = ops.approximate_cholesky_depths(*args, seed=9)
    assert torch.equal(before, after)


def test_not_grouped_is_reported(ops):
    sc = _graph_sc(path(5), 5)   # columns 0, 1, 1, 2, 2, 3, 3, 4
    bad = sc[torch.tensor([0, 1, 3, 2, 4, 5, 6, 7], device=sc.device)]   # columns 0, 1, 2, 1, ...: column 1 starts two blocks
    with pytest.raises(ValueError, match="contiguous"):
        ops.snapshot_stats(bad, [0, bad.shape[0]], 5)


def test_depths_adapter_stats(ops):
    from rlap_amd.adapters import rLapDepths
    n = 3000
    ei = cuda_ei(ba_graph(n, 5, 4))
    aug = rLapDepths(fracs=(0.1, 0.3, 0.5), views=3, seed=12)
    st = aug.stats((None, ei, None))
    assert st["max_sv"].shape == (3, 3) and st["node_count"].shape == (3, 3) and st["edge_count"].shape == (3, 3)
    runs = aug.augment((None, ei, None))
    for r in range(3):
        for k in range(3):
            e = runs[r][k]
            e = e.edge_index if hasattr(e, "edge_index") else e[1]
            assert int(st["edge_count"][r, k]) == e.shape[1]
            assert int(st["node_count"][r, k]) == torch.unique(e).numel()
            sc = torch.stack([e[0].double(), e[1].double(), torch.ones(e.shape[1], dtype=torch.float64, device=e.device)], 1)
            ref = dense_lambda(sc, n, False)
            assert abs(float(st["max_sv"][r, k]) - ref) <= 1e-9 * ref
