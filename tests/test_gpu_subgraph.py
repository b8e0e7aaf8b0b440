"""Induced subgraphs and relabelling of snapshots on the device (ops.snapshot_subgraph, rlap_snapshot_subgraph) and the adapters on
top of it (rLapChain, rLapDepths.relabelled, rLapDepths.batch_edge_counts).

The yardstick of every result is the torch formulation below, written once and independent of the code under test: per segment
ids = torch.unique(nodes or id columns), keep = isin(i, ids) & isin(j, ids) [& (i != j)], out = part[keep], labels by
torch.searchsorted(ids, .).  The feature copies weights and computes integers: every comparison is torch.equal."""
import numpy as np
import pytest
import torch

import oracle
from util import ba_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


def torch_segment(part, nodes=None, relabel=False, remove_self_loops=False):
    """(kept rows, ids) of one segment: the torch formulation."""
    i, j = part[:, 0].long(), part[:, 1].long()
    if nodes is None:
        src = part[:, :2].long()
        if remove_self_loops:
            src = src[i != j]
        ids = torch.unique(src)
    else:
        ids = torch.unique(nodes)
    keep = torch.isin(i, ids) & torch.isin(j, ids)
    if remove_self_loops:
        keep = keep & (i != j)
    out = part[keep]
    if relabel:
        out = torch.stack([torch.searchsorted(ids, i[keep]).double(), torch.searchsorted(ids, j[keep]).double(), out[:, 2]], 1)
    return out, ids


def torch_formulation(sc, ptr, nodes_of=None, **kw):
    """(out, optr, ids, iptr) of a whole call: segment s with node list nodes_of(s) (None: the ids of its rows)."""
    p = torch.as_tensor(ptr).tolist()
    outs, idss = [], []
    for s in range(len(p) - 1):
        o, d = torch_segment(sc[p[s]:p[s + 1]], None if nodes_of is None else nodes_of(s), **kw)
        outs.append(o)
        idss.append(d)
    dev = sc.device
    optr = torch.tensor([0] + list(np.cumsum([o.shape[0] for o in outs])), dtype=torch.int64, device=dev)
    iptr = torch.tensor([0] + list(np.cumsum([d.numel() for d in idss])), dtype=torch.int64, device=dev)
    out = torch.cat(outs) if outs else sc[:0]
    ids = torch.cat(idss) if idss else torch.zeros(0, dtype=torch.int64, device=dev)
    return out.reshape(-1, 3), optr, ids, iptr


def assert_call(got, ref, what=""):
    names = ("out", "optr", "ids", "iptr")
    for name, a, b in zip(names, got, ref):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name} {a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)}"
        assert torch.equal(a, b), f"{what}: {name} differs"
    # the weight column bit for bit (torch.equal on floats treats -0.0 == 0.0: compare the bytes too)
    assert torch.equal(got[0][:, 2].contiguous().view(torch.int64), ref[0][:, 2].contiguous().view(torch.int64)), f"{what}: weight bits"


def depths_views(ops, n, m, seed, o_v, ts, views=2, node_ptr=None, ei=None):
    ei = torch.from_numpy(ba_graph(n, m, seed)).cuda() if ei is None else ei
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, ts, o_v, "asc", views=views, node_ptr=node_ptr, seed=11, return_device="same")
    return sc, ptr


# ------------------------------------------------------------------------------------------------ 4. snapshots of a depths x views call
@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_depths_views_relabel(ops, o_v):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, o_v, [n // 8, n // 4, n // 2])
    assert ptr.numel() == 7
    got = ops.snapshot_subgraph(sc, ptr, n, nodes=None, relabel=True)
    assert ops.last_stats["host_syncs"] <= 2 and ops.last_stats["rows_kept"] == sc.shape[0]
    assert_call(got, torch_formulation(sc, ptr, relabel=True), f"{o_v} relabel")
    iptr = got[3]
    assert torch.equal(iptr[1:] - iptr[:-1], ops.snapshot_stats(sc, ptr, n)["nodes"])
    # without relabel every row stays as it is: both ids of every row are in the set
    out, optr, ids, iptr2 = ops.snapshot_subgraph(sc, ptr, n)
    assert torch.equal(out, sc) and torch.equal(optr.cpu(), torch.as_tensor(ptr).cpu()) and torch.equal(ids, got[2]) and torch.equal(iptr2, iptr)
    for s in range(6):   # labels are compact: every label of 0..k-1 occurs
        part = got[0][int(got[1][s]):int(got[1][s + 1]), :2].long()
        k = int(iptr[s + 1] - iptr[s])
        assert torch.equal(torch.unique(part), torch.arange(k, device=part.device))


# ------------------------------------------------------------------------------------------------ 5. subsets
@pytest.fixture(scope="module")
def snaps(ops):
    n = 3000
    sc, ptr = depths_views(ops, n, 5, 2, "random", [n // 8, n // 4, n // 2])
    return n, sc, ptr


@pytest.mark.parametrize("relabel", [False, True])
def test_one_list_for_all_segments(ops, snaps, relabel):
    n, sc, ptr = snaps
    g = torch.Generator().manual_seed(1)
    nodes = torch.randperm(n, generator=g)[:1200].cuda()
    got = ops.snapshot_subgraph(sc, ptr, n, nodes=nodes, relabel=relabel)
    assert_call(got, torch_formulation(sc, ptr, lambda s: nodes, relabel=relabel), "shared list")
    assert 0 < got[0].shape[0] < sc.shape[0]
    assert torch.equal(got[3], torch.arange(7, device="cuda") * 1200)     # ids without rows still belong to the set


def test_one_list_spanning_the_graphs_of_a_batch(ops):
    sizes = [100, 65, 63, 1, 64, 129]
    node_ptr = [0] + list(np.cumsum(sizes))
    n, sc, ptr, _ = batch_snapshots(ops, sizes)
    g = torch.Generator().manual_seed(2)
    nodes = torch.randperm(n, generator=g)[:250].cuda()
    G = len(sizes)

    def part_of_list(s):
        lo, hi = node_ptr[s % G], node_ptr[s % G + 1]
        return nodes[(nodes >= lo) & (nodes < hi)]
    for relabel in (False, True):
        got = ops.snapshot_subgraph(sc, ptr, n, nodes=nodes, node_ptr=node_ptr, relabel=relabel)
        assert_call(got, torch_formulation(sc, ptr, part_of_list, relabel=relabel), f"shared list over a batch, relabel={relabel}")


def test_a_list_per_segment(ops, snaps):
    n, sc, ptr = snaps
    p = ptr.tolist()
    g = torch.Generator().manual_seed(3)
    present = [torch.unique(sc[p[s]:p[s + 1], :2].long()) for s in range(6)]
    absent = [torch.tensor(sorted(set(range(n)) - set(present[s].tolist())), device="cuda") for s in range(6)]
    assert absent[2].numel() > 10
    lists = [
        present[0][torch.randperm(present[0].numel(), generator=g)[:500].cuda()],          # unsorted
        torch.zeros(0, dtype=torch.int64, device="cuda"),                                   # an empty list
        torch.cat([present[2][:300], absent[2][:10]]),                                      # ids that no row of the segment has
        present[3][torch.randint(0, 400, (900,), generator=g).cuda()],                      # unsorted, with repeats
        present[4],                                                                         # the whole set
        torch.tensor([n - 1, 0, n - 1], device="cuda"),
    ]
    nodes = torch.cat(lists)
    nodes_ptr = [0] + list(np.cumsum([x.numel() for x in lists]))
    for relabel in (False, True):
        got = ops.snapshot_subgraph(sc, ptr, n, nodes=nodes, nodes_ptr=nodes_ptr, relabel=relabel)
        assert_call(got, torch_formulation(sc, ptr, lambda s: lists[s], relabel=relabel), f"lists, relabel={relabel}")
        o = got[1].tolist()
        assert o[2] - o[1] == 0 and o[5] - o[4] == p[5] - p[4]
        ip = got[3].tolist()
        assert ip[3] - ip[2] == 310 and ip[2] - ip[1] == 0
        # the unsorted list with repeats gives the result of its sorted distinct form
        clean = [torch.unique(x) for x in lists]
        got2 = ops.snapshot_subgraph(sc, ptr, n, nodes=torch.cat(clean), nodes_ptr=[0] + list(np.cumsum([x.numel() for x in clean])),
                                     relabel=relabel)
        assert_call(got2, got, "sorted distinct lists")
    # the input's row order is kept: the kept rows are a subsequence of the segment
    out, optr, _, _ = ops.snapshot_subgraph(sc, ptr, n, nodes=nodes, nodes_ptr=nodes_ptr)
    for s in (0, 3):
        part, kept = sc[p[s]:p[s + 1]], out[int(optr[s]):int(optr[s + 1])]
        mask = torch.isin(part[:, 0].long(), lists[s]) & torch.isin(part[:, 1].long(), lists[s])
        assert torch.equal(part[mask], kept)


# ------------------------------------------------------------------------------------------------ 6. self loops
def test_remove_self_loops_on_a_ppr_result(ops, snaps):
    n, sc, ptr = snaps
    out, pptr = ops.snapshot_ppr(sc, ptr, n)
    assert bool((out[:, 0] == out[:, 1]).any()), "the diffusion has diagonal rows"
    for relabel in (False, True):
        got = ops.snapshot_subgraph(out, pptr, n, remove_self_loops=True, relabel=relabel)
        assert_call(got, torch_formulation(out, pptr, remove_self_loops=True, relabel=relabel), f"ppr result, relabel={relabel}")
        assert not bool((got[0][:, 0] == got[0][:, 1]).any())
    got = ops.snapshot_subgraph(out, pptr, n, relabel=True)        # and with the diagonal rows kept
    assert_call(got, torch_formulation(out, pptr, relabel=True), "ppr result with self loops")


def test_node_with_only_a_self_loop(ops):
    rows = torch.tensor([[0, 1, 0.5], [1, 0, 0.5], [7, 7, 2.0], [1, 3, 0.25], [3, 1, 0.25], [3, 3, 1.0]], dtype=torch.float64).cuda()
    got = ops.snapshot_subgraph(rows, [0, 6], 9, remove_self_loops=True, relabel=True)
    assert_call(got, torch_formulation(rows, [0, 6], remove_self_loops=True, relabel=True), "hand-made")
    assert got[2].tolist() == [0, 1, 3] and 7 not in got[2].tolist()
    assert got[0].tolist() == [[0, 1, 0.5], [1, 0, 0.5], [1, 2, 0.25], [2, 1, 0.25]]
    got = ops.snapshot_subgraph(rows, [0, 6], 9, relabel=True)
    assert got[2].tolist() == [0, 1, 3, 7] and got[0].shape[0] == 6
    # with a list the rule only drops rows: 7 is in the set because the list says so
    got = ops.snapshot_subgraph(rows, [0, 6], 9, nodes=[7, 3], remove_self_loops=True)
    assert got[2].tolist() == [3, 7] and got[0].shape[0] == 0


# ------------------------------------------------------------------------------------------------ 7. a plain edge list
def test_plain_edge_list(ops):
    """Unsymmetric, ungrouped, shuffled: snapshot_stats refuses this input (columns not contiguous / a row id without a column);
    the filter must not care."""
    rs = np.random.RandomState(5)
    n, m = 777, 6000
    rows = np.stack([rs.randint(0, n, m), rs.randint(0, n // 2, m), rs.rand(m)], 1).astype(np.float64)
    sc = torch.from_numpy(rows).cuda()
    ptr = [0, 2500, 2500, m]
    with pytest.raises(ValueError):
        ops.snapshot_stats(sc, ptr, n)
    for kw in ({"relabel": True}, {"relabel": True, "remove_self_loops": True}, {}):
        assert_call(ops.snapshot_subgraph(sc, ptr, n, **kw), torch_formulation(sc, ptr, **kw), f"edge list {kw}")
    nodes = torch.from_numpy(rs.permutation(n)[:300]).cuda()
    assert_call(ops.snapshot_subgraph(sc, ptr, n, nodes=nodes, relabel=True), torch_formulation(sc, ptr, lambda s: nodes, relabel=True),
                "edge list with a list")


# ------------------------------------------------------------------------------------------------ 8. batches
def batch_snapshots(ops, sizes, views=2):
    """Depths x views of a batch of BA graphs of the given sizes (a graph of one vertex has no edge)."""
    node_ptr = [0] + list(np.cumsum(sizes))
    parts = []
    for g, k in enumerate(sizes):
        if k >= 4:
            parts.append(ba_graph(k, 3, 40 + g) + node_ptr[g])
    # the elimination wants the union sorted by (col, row): the graphs own ascending id ranges, so concatenation keeps that order
    ei = torch.from_numpy(np.concatenate(parts, 1)).cuda()
    n = node_ptr[-1]
    G = len(sizes)
    ts = torch.tensor([[[k // 4 for k in sizes]] * views, [[k // 2 for k in sizes]] * views])
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, ts, "random", "asc", node_ptr=node_ptr, views=views, seed=4, return_device="same")
    assert ptr.numel() == 2 * views * G + 1
    return n, sc, ptr, node_ptr


def test_batches_equal_their_segments_alone(ops):
    sizes = [100, 65, 63, 1, 64, 129]
    n, sc, ptr, node_ptr = batch_snapshots(ops, sizes)
    G = len(sizes)
    p = ptr.tolist()
    for kw in ({"relabel": True}, {"relabel": False}, {"relabel": True, "remove_self_loops": True}):
        got = ops.snapshot_subgraph(sc, ptr, n, node_ptr=node_ptr, **kw)
        assert_call(got, torch_formulation(sc, ptr, **kw), f"batch {kw}")
        out, optr, ids, iptr = got
        o, ip = optr.tolist(), iptr.tolist()
        for s in range(len(p) - 1):
            g = s % G
            part = sc[p[s]:p[s + 1]].clone()
            lo = node_ptr[g]
            part[:, :2] -= lo                                    # the segment alone, as a graph of its own size
            a_out, a_optr, a_ids, a_iptr = ops.snapshot_subgraph(part, [0, part.shape[0]], sizes[g], **kw)
            mine = out[o[s]:o[s + 1]].clone()
            if not kw["relabel"]:
                mine[:, :2] -= lo
            assert torch.equal(mine, a_out) and torch.equal(ids[ip[s]:ip[s + 1]] - lo, a_ids), f"segment {s} {kw}"
            if kw["relabel"] and mine.shape[0]:
                assert int(mine[:, :2].min()) == 0               # labels restart at 0 in every segment
                assert int(mine[:, :2].max()) == ip[s + 1] - ip[s] - 1


# ------------------------------------------------------------------------------------------------ 9. edge cases
def test_edge_cases(ops):
    empty = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    out, optr, ids, iptr = ops.snapshot_subgraph(empty, [0], 10)                      # S = 0
    assert out.shape == (0, 3) and optr.tolist() == [0] and ids.numel() == 0 and iptr.tolist() == [0]
    out, optr, ids, iptr = ops.snapshot_subgraph(empty, [0, 0, 0], 10, relabel=True)  # m = 0
    assert out.shape == (0, 3) and optr.tolist() == [0, 0, 0] and ids.numel() == 0 and iptr.tolist() == [0, 0, 0]
    out, optr, ids, iptr = ops.snapshot_subgraph(empty, [0, 0], 10, nodes=[4, 2])     # m = 0 with a list: the set is still there
    assert ids.tolist() == [2, 4] and iptr.tolist() == [0, 2] and optr.tolist() == [0, 0]
    out, optr, ids, iptr = ops.snapshot_subgraph(empty, [0, 0], 0)                    # num_nodes = 0
    assert optr.tolist() == [0, 0] and iptr.tolist() == [0, 0]
    n = 131                                                                           # not a multiple of 64; the highest id present
    rows = torch.tensor([[n - 1, 0, 1.0], [0, n - 1, 1.0], [64, 63, 2.0], [63, 64, 2.0], [n - 1, 64, 3.0]], dtype=torch.float64).cuda()
    for ptr in ([0, 5], [0, 0, 2, 2, 5, 5], [0, 2, 5]):                               # segments without rows, also first and last
        for kw in ({"relabel": True}, {}):
            assert_call(ops.snapshot_subgraph(rows, ptr, n, **kw), torch_formulation(rows, ptr, **kw), f"{ptr} {kw}")
    got = ops.snapshot_subgraph(rows, [0, 5], n, relabel=True)
    assert got[2].tolist() == [0, 63, 64, n - 1] and got[0][4].tolist() == [3.0, 2.0, 3.0]
    out, optr, ids, iptr = ops.snapshot_subgraph(rows, [0, 2, 5], n, nodes=[])        # an empty node set: nothing kept
    assert out.shape == (0, 3) and optr.tolist() == [0, 0, 0] and ids.numel() == 0 and iptr.tolist() == [0, 0, 0]
    # a CPU input is copied to the device like everywhere else; the results live there
    got = ops.snapshot_subgraph(rows.cpu(), [0, 5], n, relabel=True)
    assert got[0].is_cuda and got[2].tolist() == [0, 63, 64, n - 1]


def test_tile_edges(ops):
    """Row counts around the 1,024-row tile of the filter, segment starts on and off the tile grid."""
    rs = np.random.RandomState(9)
    n = 500
    for m in (1023, 1024, 1025, 2048, 3 * 1024 + 7):
        rows = np.stack([rs.randint(0, n, m), rs.randint(0, n, m), rs.rand(m)], 1).astype(np.float64)
        sc = torch.from_numpy(rows).cuda()
        nodes = torch.from_numpy(rs.permutation(n)[:350]).cuda()
        for ptr in ([0, m], [0, 1, 1024 if m > 1024 else 512, m - 1, m], [0, 0, m, m]):
            assert_call(ops.snapshot_subgraph(sc, ptr, n, nodes=nodes, relabel=True),
                        torch_formulation(sc, ptr, lambda s: nodes, relabel=True), f"m={m} ptr={ptr}")
        # rows that do not start on a 16-byte boundary (a view that begins at an odd row)
        assert_call(ops.snapshot_subgraph(sc[1:], [0, m - 1], n, nodes=nodes, relabel=True),
                    torch_formulation(sc[1:], [0, m - 1], lambda s: nodes, relabel=True), f"m={m} odd start")


# ------------------------------------------------------------------------------------------------ 10. errors
def test_out_of_range_ids_raise_and_leave_the_process_intact(ops, snaps):
    n, sc, ptr = snaps
    good = torch.tensor([[0, 1, 1.0], [1, 0, 1.0], [2, 1, 1.0]], dtype=torch.float64).cuda()
    for bad_id in (5.0, 6.0, -1.0):
        rows = good.clone()
        rows[2, 0] = bad_id
        with pytest.raises(ValueError, match="range"):
            ops.snapshot_subgraph(rows, [0, 3], 5)
        with pytest.raises(ValueError, match="range"):
            ops.snapshot_subgraph(rows, [0, 3], 5, nodes=[0, 1], relabel=True)
    with pytest.raises(ValueError, match="range"):
        ops.snapshot_subgraph(good, [0, 3], 5, nodes=[0, 5])                     # a list id >= num_nodes
    with pytest.raises(ValueError, match="range"):
        ops.snapshot_subgraph(good, [0, 3], 5, nodes=[-1])
    # under node_ptr: rows and per-segment lists must stay inside their graph's range
    two = torch.tensor([[0, 1, 1.0], [1, 0, 1.0], [3, 4, 1.0], [4, 3, 1.0]], dtype=torch.float64).cuda()
    ok = ops.snapshot_subgraph(two, [0, 2, 4], 6, node_ptr=[0, 3, 6], nodes=[0, 1, 4, 3], nodes_ptr=[0, 2, 4], relabel=True)
    assert ok[0].tolist() == [[0, 1, 1.0], [1, 0, 1.0], [0, 1, 1.0], [1, 0, 1.0]] and ok[2].tolist() == [0, 1, 3, 4]
    with pytest.raises(ValueError, match="range"):
        ops.snapshot_subgraph(two, [0, 2, 4], 6, node_ptr=[0, 3, 6], nodes=[0, 3, 4, 3], nodes_ptr=[0, 2, 4])   # 3 in graph 0's list
    with pytest.raises(ValueError, match="range"):
        ops.snapshot_subgraph(two, [0, 1, 4], 6, node_ptr=[0, 3, 6])                                            # row (1, 0) in graph 1
    shared = ops.snapshot_subgraph(two, [0, 2, 4], 6, node_ptr=[0, 3, 6], nodes=[0, 3, 4, 3, 1])               # a shared list may span
    assert shared[0].shape[0] == 4 and shared[2].tolist() == [0, 1, 3, 4] and shared[3].tolist() == [0, 2, 4]
    # a correct call afterwards gives the right answer
    assert_call(ops.snapshot_subgraph(sc, ptr, n, relabel=True), torch_formulation(sc, ptr, relabel=True), "after the errors")


# ------------------------------------------------------------------------------------------------ 11. beyond the small regime
def test_ba_200k(ops):
    n = 200_000
    from rlap_amd import graphs
    ei = graphs.barabasi_albert(n, 8, 1).cuda()
    sc, ptr = depths_views(ops, n, 8, 1, "random", [n // 4, n // 2], ei=ei)
    got = ops.snapshot_subgraph(sc, ptr, n, relabel=True)
    assert ops.last_stats["host_syncs"] <= 2
    again = ops.snapshot_subgraph(sc, ptr, n, relabel=True)
    assert_call(again, got, "the same call twice")
    assert_call(got, torch_formulation(sc, ptr, relabel=True), "BA(200k, 8)")


# ------------------------------------------------------------------------------------------------ 12. the chain
def chain_input():
    n = 2000
    ba = ba_graph(1500, 3, 7)
    a = np.arange(1500, 2000, 2, dtype=np.int64)
    pairs = np.stack([np.concatenate([a, a + 1]), np.concatenate([a + 1, a])])
    ei = np.concatenate([ba, pairs], 1)
    ei = ei[:, np.lexsort((ei[0], ei[1]))]          # symmetric, coalesced, sorted by (col, row)
    return n, ei


def reference_chain(n, ei, o_v, rounds, t, seed, perms):
    """The chain with the CPU oracle and numpy's unique: [(rows in the input's id space, rows relabelled, node count)]."""
    res = []
    cur_ei, cur_w, cur_n, back = ei, None, n, np.arange(n)
    for k in range(rounds):
        perm = perms(k, cur_n) if perms is not None else None
        sc = oracle.approximate_cholesky(cur_ei, cur_w, cur_n, t, o_v, "asc", perm=perm, shuffle_seed=seed + k)
        ids, inv = np.unique(sc[:, :2].astype(np.int64), return_inverse=True)
        rel = np.concatenate([inv.reshape(-1, 2).astype(np.float64), sc[:, 2:3]], 1)
        back = back[ids]
        res.append((np.concatenate([back[inv.reshape(-1, 2)].astype(np.float64), sc[:, 2:3]], 1), rel, len(ids), cur_n))
        cur_ei, cur_w, cur_n = np.ascontiguousarray(rel[:, :2].T.astype(np.int64)), rel[:, 2].copy(), len(ids)
    return res


@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_chain_against_the_oracle(ops, o_v):
    from rlap_amd.adapters import Graph, rLapChain
    n, ei = chain_input()
    t = int(0.05 * n)
    perms = (lambda k, nk: np.random.RandomState(100 + k).permutation(nk)) if o_v == "random" else None
    ref = reference_chain(n, ei, o_v, 4, t, 3, perms)
    for rows, _, _, _ in ref:
        assert rows.shape[0] > 0
    # the property that makes the relabel matter: some round leaves survivors without an edge, so num_nodes_k < num_nodes_{k-1} - t
    if o_v == "random":
        assert any(nk < prev - t for _, _, nk, prev in ref), [(nk, prev) for _, _, nk, prev in ref]
    chain = rLapChain(0.05, 4, o_v, "asc", seed=3, perms=perms)
    g = Graph(None, torch.from_numpy(ei).cuda(), None)
    graphs = chain.augment(g)
    assert len(graphs) == 4 and chain.num_remove == t
    for k, (gr, (rows, _, _, _)) in enumerate(zip(graphs, ref)):
        got = torch.cat([gr.edge_index.t().double(), gr.edge_weights[:, None]], 1).cpu().numpy()
        assert got.shape == rows.shape, f"{o_v} round {k}: rows {got.shape} vs {rows.shape}"
        assert np.array_equal(got, rows), f"{o_v} round {k} differs from the oracle chain"
    st = chain.stats(g)
    assert st["node_count"].shape == (1, 4)
    assert st["node_count"][0].tolist() == [nk for _, _, nk, _ in ref]
    assert st["edge_count"][0].tolist() == [rows.shape[0] for rows, _, _, _ in ref]
    assert bool((st["max_sv"] > 0).all())


def test_chain_with_device_drawn_orders(ops):
    """Without `perms` round k is a single ops.approximate_cholesky(..., seed=3 + k) on the torch-relabelled result of round k-1."""
    from rlap_amd.adapters import Graph, rLapChain
    n, ei = chain_input()
    t = int(0.05 * n)
    ei_t = torch.from_numpy(ei).cuda()
    graphs = rLapChain(0.05, 4, "random", "asc", seed=3).augment(Graph(None, ei_t, None))
    cur_ei, cur_w, cur_n, back = ei_t, None, n, torch.arange(n, device="cuda")
    for k in range(4):
        sc = ops.approximate_cholesky(cur_ei, cur_w, cur_n, t, "random", "asc", seed=3 + k, return_device="same")
        rel, ids = torch_segment(sc, relabel=True)
        back = back[ids]
        assert torch.equal(graphs[k].edge_index, back[rel[:, :2].long()].t()), f"round {k}"
        assert torch.equal(graphs[k].edge_weights, rel[:, 2]), f"round {k}"
        cur_ei, cur_w, cur_n = rel[:, :2].long().t().contiguous(), rel[:, 2].contiguous(), int(ids.numel())


# ------------------------------------------------------------------------------------------------ 13. the rLapDepths additions
@pytest.mark.parametrize("views", [None, 2])
def test_depths_relabelled(ops, views):
    from rlap_amd.adapters import Graph, rLapDepths
    n = 1200
    g = Graph(None, torch.from_numpy(ba_graph(n, 4, 3)).cuda(), None)
    aug = rLapDepths((0.1, 0.3, 0.5), "random", "asc", keep_weights=True, seed=8, views=views)
    plain, rel = aug.augment(g), aug.relabelled(g)
    if views is None:
        plain, rel = [plain], [rel]
    assert len(rel) == len(plain)
    for run_p, run_r in zip(plain, rel):
        assert len(run_r) == 3
        for gp, (gr, ids) in zip(run_p, run_r):
            part = torch.cat([gp.edge_index.t().double(), gp.edge_weights[:, None]], 1)
            ref, ref_ids = torch_segment(part, relabel=True)
            assert torch.equal(ids, ref_ids)
            assert torch.equal(gr.edge_index, ref[:, :2].long().t()) and torch.equal(gr.edge_weights, ref[:, 2])
            assert torch.equal(ids[gr.edge_index], gp.edge_index)          # the map leads back


@pytest.mark.parametrize("views", [None, 2])
def test_depths_batch_edge_counts(ops, views):
    from rlap_amd.adapters import Graph, rLapDepths
    n = 1200
    g = Graph(None, torch.from_numpy(ba_graph(n, 4, 3)).cuda(), None)
    aug = rLapDepths((0.2, 0.5), "random", "asc", seed=8, views=views)
    counts, batches = aug.batch_edge_counts(g, 256, generator=torch.Generator().manual_seed(5))
    counts2, batches2 = aug.batch_edge_counts(g, 256, generator=torch.Generator().manual_seed(5))
    diff = aug.diffuse(g)
    if views is None:
        diff, batches, batches2 = [diff], [batches], [batches2]
    R = len(diff)
    assert counts.shape == (R, 2) and torch.equal(counts, counts2)
    for r in range(R):
        for k in range(2):
            gd, b = diff[r][k], batches[r][k]
            assert torch.equal(b, batches2[r][k])
            part = torch.cat([gd.edge_index.t().double(), gd.edge_weights[:, None]], 1)
            _, node_set = torch_segment(part, remove_self_loops=True)
            assert b.numel() == min(256, node_set.numel()) and torch.unique(b).numel() == b.numel() and bool(torch.isin(b, node_set).all())
            kept, _ = torch_segment(part, nodes=b)
            assert int(counts[r, k]) == kept.shape[0] > 0
