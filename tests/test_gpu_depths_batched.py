"""Nested Schur complements of node_ptr batches and views (ops.approximate_cholesky_depths with node_ptr / views,
rlap_approx_chol_views_depths): D depths of every (view, graph) from one elimination of the K-fold union.

Contract (include/rlap_hip.h): snapshot (d, k, g) equals approximate_cholesky on graph g alone with num_remove t[d][k][g], seed
+ k*G + g and perm slice (k, g), ids shifted by node_ptr[g] -- indices, row order and weights bit-exact, so the CPU oracle's single
call; depth row d equals approximate_cholesky_views(..., num_remove=t[d], node_ptr=...).  Every call that is not meant to retry
finishes in one attempt (n_retries == 0) on the kernel the default rule (or RLAP_FLOW) picks for K*G graphs of K*N vertices."""
import os

import numpy as np
import pytest
import torch

import oracle
from util import assert_kernel, ba_graph, clique, default_kernel, grid2d, path, star, sym_weights, symmetrize, wide_weights

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error::rlap_amd.ops.DataflowFallbackWarning")]

PAIRS = [(a, b) for a in ("random", "degree", "coarsen") for b in ("asc", "desc", "random")]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(params=["0", "1"])
def flow(request, monkeypatch):
    """RLAP_FLOW for the o_v = random calls: 0 the round kernel, 1 the dataflow kernel (the other orders always run the round kernel)."""
    monkeypatch.setenv("RLAP_FLOW", request.param)
    return int(request.param)


def expected_kernel(o_v, KG, KN):
    env = os.environ.get("RLAP_FLOW")
    if o_v == "random" and env is not None:
        return 2 if env == "1" else 1
    return default_kernel(o_v, KG, KN)


def assert_same(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, f"{what}: rows {a.shape} vs {b.shape}"
    assert np.array_equal(a[:, :2], b[:, :2]), f"{what}: indices differ"
    assert np.array_equal(a[:, 2], b[:, 2]), f"{what}: weights differ"


class Batch:
    """A ragged batch: graph g = (local edge_index, weights or None, n_g); the union's edge_index with ids shifted by node_ptr[g]."""

    def __init__(self, gs, weighted=False):
        self.gs = [(e, (np.ones(e.shape[1]) if (weighted and w is None) else w), n) for e, w, n in gs]
        self.node_ptr = np.concatenate([[0], np.cumsum([n for _, _, n in gs])]).astype(np.int64)
        self.G, self.N = len(gs), int(self.node_ptr[-1])
        self.ei = np.concatenate([e + self.node_ptr[g] for g, (e, _, _) in enumerate(self.gs)], axis=1).astype(np.int64)
        self.w = np.concatenate([w for _, w, _ in self.gs]) if weighted else None

    def perm(self, K, seed):
        rng = np.random.RandomState(seed)
        return np.concatenate([rng.permutation(n) for _ in range(K) for _, _, n in self.gs]).astype(np.int64)

    def tensors(self):
        ei = torch.from_numpy(np.ascontiguousarray(self.ei)).cuda()
        w = None if self.w is None else torch.from_numpy(self.w).cuda()
        return ei, w


def run(ops, B, t, o_v, o_n, K, *, perm=None, seed=7, mode="exact", retries_ok=False, kernel=None):
    """The depths call on batch B with the (D, K, G) table t: snapshots[d][k][g] in the input's id space."""
    t = np.asarray(t, dtype=np.int64)
    D = t.shape[0]
    ei, w = B.tensors()
    p = None if perm is None else torch.from_numpy(perm)
    sc, ptr = ops.approximate_cholesky_depths(ei, w, B.N, torch.from_numpy(t), o_v, o_n, node_ptr=torch.from_numpy(B.node_ptr), views=K,
                                              perm=p, seed=seed, mode=mode)
    st = ops.last_stats
    if not retries_ok:
        assert st["n_retries"] == 0, f"{o_v}/{o_n}: the call was repeated ({st})"
    ne = sum(max(0, min(int(t[-1, k, g]), n - 1)) for k in range(K) for g, (_, _, n) in enumerate(B.gs))
    assert st["n_eliminated"] == ne
    if ne > 0:
        assert_kernel(ops, expected_kernel(o_v, K * B.G, K * B.N) if kernel is None else kernel, f"depths {o_v}/{o_n} K={K} G={B.G}")
    sc, ptr = sc.cpu().numpy(), ptr.numpy()
    assert len(ptr) == D * K * B.G + 1 and ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and ptr[-1] == sc.shape[0] == st["out_rows"]
    return [[[sc[ptr[(d * K + k) * B.G + g]:ptr[(d * K + k) * B.G + g + 1]] for g in range(B.G)] for k in range(K)] for d in range(D)], ptr


def check_oracle(snaps, B, t, o_v, o_n, K, what, *, perm=None, seed=7, mode="exact"):
    t = np.asarray(t)
    for d in range(t.shape[0]):
        for k in range(K):
            for g, (e, w, n) in enumerate(B.gs):
                got = snaps[d][k][g].copy()
                got[:, :2] -= B.node_ptr[g]
                if n == 0:
                    assert got.shape[0] == 0
                    continue
                pk = None if perm is None else perm[k * B.N + B.node_ptr[g]:k * B.N + B.node_ptr[g + 1]]
                ref = oracle.approximate_cholesky(e, w, n, int(t[d, k, g]), o_v, o_n, perm=pk, shuffle_seed=seed + k * B.G + g, mode=mode)
                assert_same(got, ref, f"{what} {o_v}/{o_n} snapshot (d={d}, k={k}, g={g}, t={int(t[d, k, g])}, n={n}) vs oracle")


def check_views(ops, snaps, ptr, B, t, o_v, o_n, K, what, *, perm=None, seed=7, mode="exact"):
    """Depth row d against the views call with num_remove = t[d]: rows and per-(view, graph) pointers."""
    ei, w = B.tensors()
    p = None if perm is None else torch.from_numpy(perm)
    KG = K * B.G
    for d in range(len(t)):
        sc, vp = ops.approximate_cholesky_views(ei, w, B.N, torch.from_numpy(np.asarray(t[d], dtype=np.int64)), o_v, o_n,
                                                node_ptr=torch.from_numpy(B.node_ptr), perm=p, seed=seed, mode=mode)
        assert ops.last_stats["n_retries"] == 0
        sc, vp = sc.cpu().numpy(), vp.numpy()
        assert np.array_equal(ptr[d * KG:(d + 1) * KG + 1] - ptr[d * KG], vp), f"{what}: depth {d} row pointers differ from the views call"
        assert_same(np.concatenate([snaps[d][k][g] for k in range(K) for g in range(B.G)]), sc, f"{what} {o_v}/{o_n} depth {d} vs views")


def depth_table(B, K, D, seed):
    """(D, K, G): columns that differ per graph and per view, with zeros, equal neighbours and values beyond n_g - 1."""
    rng = np.random.RandomState(seed)
    t = np.zeros((D, K, B.G), dtype=np.int64)
    for k in range(K):
        for g, (_, _, n) in enumerate(B.gs):
            col = np.sort(rng.randint(0, n + 4, size=D))
            if rng.rand() < 0.3:
                col[0] = 0
            if D > 1 and rng.rand() < 0.4:
                col[1] = col[0]
            t[:, k, g] = col
    return t


def small_batches():
    return {
        1: Batch([(ba_graph(250, 4, 3), None, 250)]),
        3: Batch([(np.zeros((2, 0), dtype=np.int64), None, 1), (ba_graph(200, 3, 4), None, 200), (grid2d(5, 6), None, 30)]),
        7: Batch([(ba_graph(300, 4, 5), None, 300), (path(40), None, 40), (np.zeros((2, 0), dtype=np.int64), None, 0), (star(30), None, 30),
                  (path(2), None, 2), (clique(12), None, 12), (grid2d(6, 7), None, 42)]),
    }


@pytest.mark.parametrize("G,K,D", [(1, 2, 3), (3, 1, 4), (3, 3, 2), (7, 2, 3)])
def test_every_pair_matches_the_oracle_per_snapshot(ops, flow, G, K, D):
    B = small_batches()[G]
    t = depth_table(B, K, D, 10 * G + K)
    for o_v, o_n in PAIRS:
        if flow == 1 and o_v != "random":
            continue   # (the round kernel's orders run once, under RLAP_FLOW=0)
        perm = B.perm(K, G + K) if o_v == "random" else None
        snaps, _ = run(ops, B, t, o_v, o_n, K, perm=perm, seed=11)
        check_oracle(snaps, B, t, o_v, o_n, K, f"G={G} K={K}", perm=perm, seed=11)


def test_wide_weights_and_unsorted_duplicate_input(ops, flow):
    gs = [(ba_graph(300, 5, 7), None, 300), (grid2d(8, 9), None, 72), (star(40), None, 40)]
    Bw = Batch([(e, wide_weights(e, n, 3 + g, 6), n) for g, (e, _, n) in enumerate(gs)], weighted=True)
    t = depth_table(Bw, 2, 3, 5)
    for o_v, o_n in (("random", "asc"), ("degree", "desc")):
        if flow == 1 and o_v != "random":
            continue
        perm = Bw.perm(2, 6) if o_v == "random" else None
        snaps, _ = run(ops, Bw, t, o_v, o_n, 2, perm=perm, seed=3)
        check_oracle(snaps, Bw, t, o_v, o_n, 2, "wide weights", perm=perm, seed=3)
    # the same batch given unsorted (equal to the sorted input's rows), and with duplicated edges in both directions (summed, like
    # every other call: equal to the views call on that input)
    Bs = Batch([(e, sym_weights(e, n, 9 + g), n) for g, (e, _, n) in enumerate(gs)], weighted=True)
    rng = np.random.RandomState(4)
    order = rng.permutation(Bs.ei.shape[1])
    sel = rng.choice(Bs.ei.shape[1], 200, replace=False)
    Bu = Batch(Bs.gs, weighted=True)
    Bu.ei, Bu.w = Bs.ei[:, order], Bs.w[order]
    Bd = Batch(Bs.gs, weighted=True)
    Bd.ei = np.concatenate([Bu.ei, Bs.ei[:, sel], Bs.ei[::-1, sel]], axis=1)
    Bd.w = np.concatenate([Bu.w, Bs.w[sel], Bs.w[sel]])
    for o_v, o_n in (("random", "random"), ("coarsen", "asc")):
        if flow == 1 and o_v != "random":
            continue
        perm = Bs.perm(2, 8) if o_v == "random" else None
        got, _ = run(ops, Bu, t, o_v, o_n, 2, perm=perm, seed=5)
        check_oracle(got, Bs, t, o_v, o_n, 2, "unsorted input", perm=perm, seed=5)
        dup, ptr = run(ops, Bd, t, o_v, o_n, 2, perm=perm, seed=5)
        check_views(ops, dup, ptr, Bd, t, o_v, o_n, 2, "duplicated edges", perm=perm, seed=5)


def test_depth_rows_equal_the_views_call(ops, flow):
    B = small_batches()[7]
    t = depth_table(B, 2, 3, 77)
    cases = [("random", "asc", None, "exact"), ("random", "random", None, "frontier"), ("degree", "asc", None, "frontier"), ("coarsen", "random", None, "exact")]
    for o_v, o_n, perm, mode in cases:
        if flow == 1 and o_v != "random":
            continue
        snaps, ptr = run(ops, B, t, o_v, o_n, 2, perm=perm, seed=21, mode=mode)   # (o_v = random: the node_id vectors drawn on the device)
        check_views(ops, snaps, ptr, B, t, o_v, o_n, 2, f"views {mode}", perm=perm, seed=21, mode=mode)


def test_one_view_one_graph_equals_the_depths_call(ops, flow):
    n = 1200
    ei = torch.from_numpy(ba_graph(n, 6, 13)).cuda()
    ts = [n // 8, n // 8, n // 3, n - 1]
    for o_v, o_n in (("random", "asc"), ("degree", "asc")):
        if flow == 1 and o_v != "random":
            continue
        a, pa = ops.approximate_cholesky_depths(ei, None, n, ts, o_v, o_n, seed=6)
        assert ops.last_stats["n_retries"] == 0
        b, pb = ops.approximate_cholesky_depths(ei, None, n, torch.tensor(ts).reshape(-1, 1, 1), o_v, o_n, seed=6)   # the new path
        assert ops.last_stats["n_retries"] == 0
        assert_kernel(ops, expected_kernel(o_v, 1, n), "K = G = 1")
        assert torch.equal(pa, pb)
        assert_same(a.cpu().numpy(), b.cpu().numpy(), f"K = G = 1 {o_v}/{o_n}")


def test_dataflow_batch_round_batch_and_config5_shape(ops):
    # <= 64 graphs of >= 1024 vertices: the default rule sends o_v = random to the dataflow kernel
    B = Batch([(ba_graph(1100 + 50 * g, 5, 30 + g), None, 1100 + 50 * g) for g in range(6)])
    assert default_kernel("random", 2 * B.G, 2 * B.N) == 2
    t = depth_table(B, 2, 3, 31)
    perm = B.perm(2, 32)
    snaps, ptr = run(ops, B, t, "random", "asc", 2, perm=perm, seed=4)
    check_oracle(snaps, B, t, "random", "asc", 2, "dataflow batch", perm=perm, seed=4)
    check_views(ops, snaps, ptr, B, t, "random", "asc", 2, "dataflow batch", perm=perm, seed=4)
    # more than 64 graphs: the round kernel
    B = Batch([(ba_graph(120 + g, 3, 40 + g), None, 120 + g) for g in range(70)])
    assert default_kernel("random", B.G, B.N) == 1
    t = depth_table(B, 1, 3, 41)
    snaps, ptr = run(ops, B, t, "random", "asc", 1, seed=4)
    check_views(ops, snaps, ptr, B, t, "random", "asc", 1, "round batch", seed=4)
    # a config-5-shaped batch: 256 x BA(4096, 8), depths [n/8, n/4, n/2]
    n = 4096
    e = ba_graph(n, 8, 1)
    B = Batch([(e, None, n)] * 256)
    t = np.repeat(np.array([n // 8, n // 4, n // 2])[:, None, None], B.G, axis=2)
    perm = B.perm(1, 9)
    snaps, ptr = run(ops, B, t, "random", "asc", 1, perm=perm, seed=9)
    check_views(ops, snaps, ptr, B, t, "random", "asc", 1, "config-5 shape", perm=perm, seed=9)
    for g in (0, 255):   # (two graphs against the oracle)
        Bg = Batch([(e, None, n)])
        check_oracle([[[snaps[d][0][g] - np.array([B.node_ptr[g], B.node_ptr[g], 0])]] for d in range(3)], Bg, t[:, :, g:g + 1], "random", "asc", 1,
                     f"config-5 shape graph {g}", perm=perm[B.node_ptr[g]:B.node_ptr[g + 1]], seed=9 + g)


def test_growth_retry_in_a_later_segment(ops, flow):
    """A uniform table that holds the first depth's draws and no more: the overflow strikes in a later segment, the whole call is
    repeated from depth 0 (retry kind 3) and every snapshot is unchanged."""
    from rlap_amd import _lib
    B = Batch([(ba_graph(1500, 6, 50 + g), None, 1500) for g in range(3)])
    t = np.array([150, 400, 750])[:, None, None] * np.ones((1, 2, B.G), dtype=np.int64)
    perm = B.perm(2, 51)
    for o_v, o_n in (("random", "asc"), ("degree", "asc")):
        if flow == 1 and o_v != "random":
            continue
        p = perm if o_v == "random" else None
        base, _ = run(ops, B, t, o_v, o_n, 2, perm=p, seed=3)
        ei, w = B.tensors()
        pt = None if p is None else torch.from_numpy(p)
        d = []
        for row in (t[0], t[-1]):
            ops.approximate_cholesky_views(ei, w, B.N, torch.from_numpy(row), o_v, o_n, node_ptr=torch.from_numpy(B.node_ptr), perm=pt, seed=3)
            d.append(ops.last_stats["n_draws"])
        assert d[1] > d[0] + 1024
        ops.debug_set_limits(rng_len=d[0] + 64)
        try:
            got, _ = run(ops, B, t, o_v, o_n, 2, perm=p, seed=3, retries_ok=True)
            st = ops.last_stats
        finally:
            ops.debug_set_limits()
        assert st["n_retries"] == 1 and st["retry_causes"] == _lib.RETRY_RNG, st
        for dd in range(len(t)):
            for k in range(2):
                for g in range(B.G):
                    assert_same(got[dd][k][g], base[dd][k][g], f"rng retry {o_v} ({dd}, {k}, {g})")


def test_reorder_fallback_moves_the_call_to_the_round_kernel(ops, monkeypatch):
    """Hubs that collect many out-of-order appended entries and survive every depth, a reorder buffer of one entry: the first
    snapshot's tag-order pass cannot hold them (retry kind 7, quiet), the whole call moves to the round kernel, rows unchanged."""
    from rlap_amd import _lib
    monkeypatch.setenv("RLAP_FLOW", "1")
    n = 1500
    a0 = np.concatenate([np.zeros(n - 2, dtype=np.int64), np.ones(n - 2, dtype=np.int64), np.arange(2, n - 1)])
    b0 = np.concatenate([np.arange(2, n), np.arange(2, n), np.arange(3, n)])
    hub = symmetrize(a0, b0, n)
    B = Batch([(hub, None, n), (ba_graph(n, 5, 60), None, n)])
    rng = np.random.RandomState(12)
    perm = np.concatenate([np.concatenate([[0, 1], 2 + rng.permutation(n - 2)]), rng.permutation(n)] * 2).astype(np.int64)   # the hubs go last
    t = np.array([n // 4, n // 2, n - 3])[:, None, None] * np.ones((1, 2, 2), dtype=np.int64)
    ops.debug_set_flow_limits(1)
    got, _ = run(ops, B, t, "random", "asc", 2, perm=perm, seed=3, retries_ok=True, kernel=_lib.KERNEL_ROUND)
    st = ops.last_stats
    assert st["retry_causes"] == _lib.RETRY_FLOW_REORDER and st["flow_abort"] == 0 and st["n_retries"] == 1, st
    check_oracle(got, B, t, "random", "asc", 2, "reorder fallback", perm=perm, seed=3)
    again, _ = run(ops, B, t, "random", "asc", 2, perm=perm, seed=3)   # (the limit held for one attempt only)
    for d in range(3):
        for k in range(2):
            for g in range(2):
                assert_same(again[d][k][g], got[d][k][g], f"dataflow again ({d}, {k}, {g})")


def test_poison_and_jitter(ops, flow):
    B = Batch([(ba_graph(1200, 6, 70 + g), None, 1200) for g in range(3)])
    t = depth_table(B, 2, 3, 71)
    perm = B.perm(2, 72)
    cases = [("random", "asc")] + ([("degree", "asc"), ("coarsen", "random")] if flow == 0 else [])
    base = {c: run(ops, B, t, *c, 2, perm=perm if c[0] == "random" else None, seed=3)[0] for c in cases}
    ops.debug_set_poison(0xA5)
    ops.debug_set_jitter(8)
    try:
        for c in cases:
            got, _ = run(ops, B, t, *c, 2, perm=perm if c[0] == "random" else None, seed=3)
            for d in range(len(t)):
                for k in range(2):
                    for g in range(B.G):
                        assert_same(got[d][k][g], base[c][d][k][g], f"poison + jitter {c} ({d}, {k}, {g})")
    finally:
        ops.debug_set_poison(-1)
        ops.debug_set_jitter(0)


def test_asymmetric_input_and_bad_c_abi_arguments(ops):
    from rlap_amd import _lib
    B = Batch([(path(20), None, 20), (path(30), None, 30)])
    ei = torch.from_numpy(B.ei[:, :-1].copy()).cuda()   # one direction of an edge dropped
    with pytest.raises(ValueError):
        ops.approximate_cholesky_depths(ei, None, B.N, [3, 6], "degree", "asc", node_ptr=B.node_ptr.tolist(), views=2)
    lib = _lib.load()
    ei = torch.from_numpy(B.ei).cuda()
    row, col = ei[0].contiguous(), ei[1].contiguous()
    out = torch.empty((4 * ei.shape[1], 3), dtype=torch.float64, device="cuda")
    ptr = torch.zeros(2 * 2 * 2 + 1, dtype=torch.int64)
    npt = torch.from_numpy(B.node_ptr)
    h = ops._handle(ei.device)[1]
    t = torch.tensor([[5, 3, 9, 9], [4, 6, 9, 9]], dtype=torch.int64)   # column 0 decreases
    args = lambda tt, K, D: (h, row.data_ptr(), col.data_ptr(), None, ei.shape[1], 2, npt.data_ptr(), K, D, tt, 1, 0, None, 0,   # noqa: E731
                             out.data_ptr(), out.shape[0], ptr.data_ptr(), None)
    assert lib.rlap_approx_chol_views_depths(*args(t.data_ptr(), 2, 2)) == 3
    assert lib.rlap_approx_chol_views_depths(*args(None, 2, 2)) == 3
    assert lib.rlap_approx_chol_views_depths(*args(t.data_ptr(), 2, 0)) == 3
    good = torch.tensor([[3, 3, 9, 9], [4, 6, 9, 9]], dtype=torch.int64)
    assert lib.rlap_approx_chol_views_depths(*args(good.data_ptr(), 2, 2)) == 0


def test_adapter_views(ops):
    from rlap_amd import adapters
    n = 1300
    ei = torch.from_numpy(ba_graph(n, 5, 2)).cuda()
    x = torch.zeros(n, 4, device="cuda")
    fracs = (0.1, 0.3, 0.6)
    runs = adapters.rLapDepths(fracs=fracs, o_v="random", o_n="asc", keep_weights=True, seed=8, views=3).augment((x, ei, None))
    assert ops.last_stats["n_retries"] == 0
    assert_kernel(ops, expected_kernel("random", 3, 3 * n), "rLapDepths(views=3)")
    assert len(runs) == 3 and all(len(r) == 3 for r in runs)
    for r in range(3):
        for k, f in enumerate(fracs):
            a = ops.approximate_cholesky(ei, None, n, int(f * n), "random", "asc", seed=8 + r, return_device="same")
            assert ops.last_stats["n_retries"] == 0
            g = runs[r][k]
            assert torch.equal(g.edge_index, a[:, :2].long().t()) and torch.equal(g.edge_weights, a[:, 2]), (r, f)
