"""The plan buffer the device builds (ops.snapshot_plan, rlap_plan.hip's k_pl_count / k_pl_fill / k_pl_fill_walk / k_pl_dir), read
through its public format and compared with an independent construction -- not through the product y.

tests/plan_buffer.py decodes the buffer by the descriptor's offsets alone (its decoder is checked against the layout header in
tests/test_plan_buffer_cpu.py) and builds every list the plain way from sc.cpu().  Nothing here has a tolerance: offsets, ids, the
zero words and the directory are integers, and a coefficient must have the bits of the float64 value that ops.snapshot_gcn_norm
gives the same entry with the same flags (tests/test_gpu_gcn_norm.py ties those to the torch formulation within its derived
bound).  A failure names the part: off[], the ids of one slot's list, the zero words, the directory, a coefficient, loopc[]."""
import ctypes

import numpy as np
import pytest
import torch

import plan_buffer
from test_gpu_plan import HAND, check_plan, depths_views, mirror, ops, star, two_stars  # noqa: F401  (mirror, ops are fixtures)
from util import ba_graph

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def build(ops, sc, ptr, n, node_ptr, directions, poison, kw):
    try:
        ops.debug_set_poison(poison)
        plan = ops.snapshot_plan(sc, ptr, n, node_ptr=node_ptr, directions=directions, **kw)
    finally:
        ops.debug_set_poison(-1)
    return plan, plan_buffer.decode(plan.buffer.cpu().numpy(), plan.desc)


def check_buffer(ops, C, sc, ptr, n, what, node_ptr=None, directions="both", **kw):
    """Everything the format promises for one input and one set of flags.  Returns the plan built over 0xFF bytes."""
    plan, dec = build(ops, sc, ptr, n, node_ptr, directions, 0xFF, kw)
    _, dec0 = build(ops, sc, ptr, n, node_ptr, directions, 0x00, kw)
    assert plan_buffer.same_decoded(dec, dec0), f"{what}: the buffer's content depends on what the buffer held before the build"
    desc, info = plan.desc, plan.info
    rows = sc.detach().cpu().double().numpy()
    p = [int(v) for v in torch.as_tensor(ptr).tolist()]
    G = len(node_ptr) - 1 if node_ptr is not None else 1
    loops = kw.get("add_self_loops", True)
    slots = ((len(p) - 1) // G) * n
    assert dec["slots"] == slots and int(desc.magic) == 0x504C414E and int(desc.m) == rows.shape[0]
    # the bytes in use
    assert int(desc.plan_bytes) == plan.nbytes == plan.buffer.numel(), what
    for name, lo, hi in dec["spans"]:
        assert 0 <= lo <= hi <= int(desc.plan_bytes), (what, name, lo, hi)
    # the coefficients of the same flags, and where the documented order of that call puts every row and every loop
    ei, val, eptr = ops.snapshot_gcn_norm(sc, ptr, n, node_ptr=node_ptr, dtype=torch.float64, **kw)
    ei, val = ei.cpu().numpy(), val.cpu().numpy()
    row_at, loop_at, e = plan_buffer.entry_numbers(rows, p, n, G, node_ptr, loops)
    assert e == eptr.tolist() and e[-1] == val.shape[0], what
    stay = row_at >= 0
    assert np.array_equal(ei[0, row_at[stay]], rows[stay, 0].astype(np.int64)) and np.array_equal(ei[1, row_at[stay]], rows[stay, 1].astype(np.int64))
    if loops:
        ids = np.tile(np.arange(n), slots // n) if n else np.zeros(0, dtype=np.int64)
        assert np.array_equal(ei[0, loop_at], ids) and np.array_equal(ei[1, loop_at], ids)
        assert dec["loopc"] is not None and np.array_equal(bits(dec["loopc"]), bits(val[loop_at])), f"{what}: loopc[]"
    else:
        assert dec["loopc"] is None and int(desc.loop_offset) == -1
    built = {"forward": directions in ("both", "forward"), "transposed": directions in ("both", "transposed")}
    for t, (name, _) in enumerate(plan_buffer.DIRECTIONS):
        d = dec[name]
        if not built[name]:
            assert d is None and info["chunked_lists_" + name] == -1, (what, name)
            for field in ("off_", "dir_", "rec_", "entries_", "chunks_"):
                assert int(getattr(desc, field + name)) == -1, (what, field + name)
            continue
        tag = f"{what} {name}"
        off = d["off"]
        assert off[0] == 0, tag
        assert bool((np.diff(off) >= 0).all()), f"{tag}: off[] decreases"
        assert off[slots] == int(getattr(desc, "entries_" + name)) == d["entries"], f"{tag}: off[slots]"
        assert int(off[slots]) + (slots if loops else 0) == plan.entries, tag
        lists = plan_buffer.expected_lists(rows, p, n, G, loops, bool(t))
        assert not lists or (min(lists) >= 0 and max(lists) < slots)
        want_len = np.zeros(slots, dtype=np.int64)
        for slot, l in lists.items():
            want_len[slot] = len(l)
        got_len = np.diff(off)
        wrong = np.nonzero(got_len != want_len)[0]
        assert wrong.size == 0, f"{tag}: slot {wrong[:4].tolist()} has {got_len[wrong[:4]].tolist()} records, not {want_len[wrong[:4]].tolist()}"
        order = [pair for slot in sorted(lists) for pair in lists[slot]]
        want_rows = np.array([r for r, _ in order], dtype=np.int64)
        want_ids = np.array([i for _, i in order], dtype=np.int32)
        if not np.array_equal(d["id"], want_ids):
            at = int(np.nonzero(d["id"] != want_ids)[0][0])
            slot = int(np.searchsorted(off, at, side="right")) - 1
            raise AssertionError(f"{tag}: record {at} (slot {slot}, place {at - int(off[slot])}) takes id {int(d['id'][at])}, not {int(want_ids[at])}")
        assert not d["zero"].any(), f"{tag}: {int(np.count_nonzero(d['zero']))} zero words are not 0"
        assert bool((row_at[want_rows] >= 0).all())
        want_c = val[row_at[want_rows]]
        if not np.array_equal(bits(d["c"]), bits(want_c)):
            at = int(np.nonzero(bits(d["c"]) != bits(want_c))[0][0])
            raise AssertionError(f"{tag}: record {at} has coefficient {d['c'][at]!r}, snapshot_gcn_norm gives row {int(want_rows[at])} {want_c[at]!r}")
        want_dir = plan_buffer.expected_directory(lists, C)
        assert d["chunks"] == int(getattr(desc, "chunks_" + name)) == len(want_dir), f"{tag}: chunks"
        assert list(zip(d["dir_slot"].tolist(), d["dir_k"].tolist())) == want_dir, f"{tag}: the directory"
        assert info["chunked_lists_" + name] == sum(1 for l in lists.values() if len(l) > C), f"{tag}: long lists"
    return plan


# ------------------------------------------------------------------------------------------------ 1. elimination results
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_depths_views(ops, mirror, o_v, weighted):
    n = 300
    sc, ptr = depths_views(ops, n, 3, 2, o_v, [75, 150], views=2)
    assert ptr.numel() == 5
    plan = check_buffer(ops, mirror.spmm_chunk(), sc, ptr, n, f"{o_v} weighted={weighted}", weighted=weighted)
    assert plan.info["loops_removed"] == 0 and plan.desc.entries_forward == plan.desc.entries_transposed == sc.shape[0]


@pytest.mark.parametrize("kw", [{"fill_value": 2.0}, {"fill_value": 2.0, "weighted": True}, {"add_self_loops": False},
                                {"add_self_loops": False, "weighted": True}, {"normalize": False}, {"normalize": False, "weighted": True},
                                {"add_self_loops": False, "normalize": False}, {"add_self_loops": False, "normalize": False, "weighted": True}])
def test_fill_value_and_switches(ops, mirror, kw):
    n = 300
    sc, ptr = depths_views(ops, n, 3, 2, "random", [75, 150], views=2)
    check_buffer(ops, mirror.spmm_chunk(), sc, ptr, n, f"{kw}", **kw)


@pytest.mark.parametrize("directions", ["forward", "transposed"])
def test_one_direction(ops, mirror, directions):
    n = 300
    sc, ptr = depths_views(ops, n, 3, 2, "random", [75, 150], views=2)
    C = mirror.spmm_chunk()
    one = check_buffer(ops, C, sc, ptr, n, directions, directions=directions, weighted=True)
    both = ops.snapshot_plan(sc, ptr, n, weighted=True)
    assert one.nbytes < both.nbytes and int(one.desc.flags) & (256 | 512) == (256 if directions == "forward" else 512)
    sc2, ptr2, n2 = two_stars(2 * C + 40)
    check_buffer(ops, C, sc2, ptr2, n2, f"stars {directions}", directions=directions, weighted=True)


@pytest.mark.parametrize("weighted", [False, True])
def test_node_ptr_batch_of_unequal_graphs(ops, mirror, weighted):
    sizes, views = [100, 65, 63, 1, 64, 129], 2
    node_ptr = [0] + [int(v) for v in np.cumsum(sizes)]
    parts = [ba_graph(k, 3, 40 + g) + node_ptr[g] for g, k in enumerate(sizes) if k >= 4]
    ei = torch.from_numpy(np.concatenate(parts, 1)).cuda()
    n = node_ptr[-1]
    ts = torch.tensor([[[k // 4 for k in sizes]] * views, [[k // 2 for k in sizes]] * views])
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, ts, "random", "asc", node_ptr=node_ptr, views=views, seed=4, return_device="same")
    assert ptr.numel() == 2 * views * len(sizes) + 1
    plan = check_buffer(ops, mirror.spmm_chunk(), sc, ptr, n, f"batch weighted={weighted}", node_ptr=node_ptr, weighted=weighted)
    assert plan.layers == 4
    check_buffer(ops, mirror.spmm_chunk(), sc, ptr, n, "batch, no loops", node_ptr=node_ptr, weighted=weighted, add_self_loops=False)


def test_num_nodes_larger_than_the_eliminations(ops, mirror):
    n = 300
    sc, ptr = depths_views(ops, n, 3, 2, "degree", [75, 150], views=2)
    plan = check_buffer(ops, mirror.spmm_chunk(), sc, ptr, n + 37, "num_nodes + 37", weighted=True)
    dec = plan_buffer.decode(plan.buffer.cpu().numpy(), plan.desc)
    for layer in range(4):                                                     # trailing ids: no record, loop coefficient exactly 1
        lo, hi = layer * (n + 37) + n, (layer + 1) * (n + 37)
        assert bool((dec["loopc"][lo:hi] == 1.0).all())
        assert dec["forward"]["off"][lo] == dec["forward"]["off"][hi] and dec["transposed"]["off"][lo] == dec["transposed"]["off"][hi]
    check_buffer(ops, mirror.spmm_chunk(), sc, ptr, n + 37, "num_nodes + 37, no loops", weighted=True, add_self_loops=False)


# ------------------------------------------------------------------------------------------------ 2. long lists, loop rows
@pytest.mark.parametrize("weighted", [False, True])
def test_two_stars_longer_than_two_chunks(ops, mirror, weighted):
    C = mirror.spmm_chunk()
    sc, ptr, n = two_stars(2 * C + 40)
    plan = check_buffer(ops, C, sc, ptr, n, f"stars weighted={weighted}", weighted=weighted)
    assert plan.desc.chunks_forward == 6 and plan.desc.chunks_transposed == 6
    dec = plan_buffer.decode(plan.buffer.cpu().numpy(), plan.desc)
    for name in ("forward", "transposed"):                                     # the centres are ids 0 of the two layers
        assert list(zip(dec[name]["dir_slot"].tolist(), dec[name]["dir_k"].tolist())) == [(0, 0), (0, 1), (0, 2), (n, 0), (n, 1), (n, 2)]


@pytest.mark.parametrize("weighted", [False, True])
def test_star_with_loop_rows(ops, mirror, weighted):
    """Loop rows inside a long block (k_pl_fill_walk): an entry's place in its list is no longer its place in its block."""
    C = mirror.spmm_chunk()
    leaves = 2 * C + 40
    a = star(leaves, 4, loops=[(3, 2.5), (C, 0.75), (C + 20, 1.25)])
    extra = np.array([[1, 1, 3.0]])                                          # a leaf's loop row, at the end of its block
    a = np.concatenate([a[:leaves + 3 + 1], extra, a[leaves + 3 + 1:]])
    sc = torch.from_numpy(np.concatenate([a, star(leaves, 5)])).cuda()
    ptr, n = [0, len(a), len(a) + 2 * leaves], leaves + 3
    plan = check_buffer(ops, C, sc, ptr, n, f"star with loop rows weighted={weighted}", weighted=weighted)
    assert plan.info["loops_removed"] == 4 and plan.desc.entries_forward == 4 * leaves == plan.desc.entries_transposed
    plan = check_buffer(ops, C, sc, ptr, n, "star, loop rows kept", weighted=weighted, add_self_loops=False)
    assert plan.info["loops_removed"] == 0 and plan.desc.entries_forward == sc.shape[0]
    short = torch.from_numpy(star(C, 6, loops=[(5, 2.0)])).cuda()             # C + 1 rows of which one is a loop row: no chunk
    plan = check_buffer(ops, C, short, [0, 2 * C + 1], C + 1, "C entries and a loop row", weighted=weighted)
    assert plan.desc.chunks_forward == 0 and plan.desc.chunks_transposed == 0


@pytest.mark.parametrize("weighted", [False, True])
def test_hand_built_input_twice_with_empty_segments(ops, mirror, weighted):
    C = mirror.spmm_chunk()
    rows = torch.tensor(HAND, dtype=torch.float64).cuda()
    two = torch.cat([rows, rows])
    plan = check_buffer(ops, C, two, [0, 8, 16], 7, "hand-built twice", weighted=weighted)
    assert plan.info["loops_removed"] == 8 and plan.entries == 2 * (8 - 4 + 7)
    check_buffer(ops, C, two, [0, 0, 8, 8, 16, 16], 7, "hand-built with empty segments", weighted=weighted, fill_value=2.0)
    check_buffer(ops, C, two, [0, 8, 16], 7, "hand-built, loops kept", weighted=weighted, add_self_loops=False)
    check_buffer(ops, C, two, [0, 8, 16], 7, "hand-built, weights as they are", weighted=weighted, normalize=False)
    empty = torch.zeros((0, 3), dtype=torch.float64, device="cuda")
    plan = check_buffer(ops, C, empty, [0, 0, 0], 5, "m = 0")
    assert plan.entries == 10


# ------------------------------------------------------------------------------------------------ 3. the trimmed buffer
def test_buffer_trimmed_to_a_storage_of_its_own(ops, mirror):
    """A path whose every id carries eight loop rows: the records that stay are a fifth of the rows, so less than 3/4 of the bound
    is in use and snapshot_plan copies the used bytes into a storage of exactly that size."""
    from rlap_amd import _lib
    n, rs = 40, np.random.RandomState(9)
    rows = []
    for j in range(n):
        block = [[i, j, 0.5 + rs.rand()] for i in (j - 1, j + 1) if 0 <= i < n]
        for k in range(8):
            block.insert(int(rs.randint(0, len(block) + 1)), [j, j, 1.0 + k + rs.rand()])
        rows += block
    sc = torch.tensor(rows, dtype=torch.float64).cuda()
    m, ptr = len(rows), [0, len(rows)]
    assert m == 2 * (n - 1) + 8 * n
    bound = ctypes.c_size_t()
    assert _lib.load().rlap_snapshot_plan_bytes(m, 1, 1, n, _lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE | _lib.GCN_WEIGHTED, ctypes.byref(bound)) == 0
    plan = check_buffer(ops, mirror.spmm_chunk(), sc, ptr, n, "path with eight loop rows an id", weighted=True)
    assert 4 * plan.nbytes < 3 * bound.value, "a condition of this test: the branch that copies is the one taken"
    assert plan.buffer.untyped_storage().nbytes() == plan.nbytes == int(plan.desc.plan_bytes) and plan.buffer.storage_offset() == 0
    assert plan.info["loops_removed"] == 8 * n and plan.desc.entries_forward == 2 * (n - 1)
    check_plan(ops, sc, ptr, n, "trimmed plan", Fs=(3, 64), plan=plan, weighted=True)
