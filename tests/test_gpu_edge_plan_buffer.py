"""The plan buffer the edge build writes (ops.edge_list_plan, rlap_edgeplan.hip's k_ep_count / k_ep_fill / k_ep_fill_walk / k_ep_dir),
read through its public format and compared with the plain Python construction of tests/plan_buffer.py -- every list by appending in
input order -- not through the product and not through the host mirror.  Nothing here has a tolerance: offsets, ids, zero words and
the directory are integers.  The coefficients are tied to the mirror in tests/test_gpu_edge_plan.py; here a record's coefficient
must be the bits of the float64 value the torch formulation's own degree gives only where that is exact (unweighted input: integer
degrees, 1 / sqrt and two products, correctly rounded on both sides)."""
import ctypes

import numpy as np
import pytest
import torch

import plan_buffer
from test_gpu_edge_plan import HAND_A, HAND_B, comb, decode, elim, ops, shuffled  # noqa: F401  (elim, ops are fixtures)

pytestmark = pytest.mark.gpu

CHUNK = 256   # (rlap_spmm.h's CHUNK, documented in include/rlap_hip.h)


def check_format(ops, rows, ptr, n, what, node_ptr=None, directions="both", **kw):
    plan = ops.edge_list_plan(rows, ptr, n, node_ptr=node_ptr, directions=directions, **kw)
    dec, desc, info = decode(plan), plan.desc, plan.info
    host = rows.detach().cpu().double().numpy()
    p = [int(v) for v in ptr]
    G = len(node_ptr) - 1 if node_ptr is not None else 1
    loops = kw.get("add_self_loops", True)
    slots = ((len(p) - 1) // G) * n
    nloop = int((host[:, 0] == host[:, 1]).sum())
    drop = loops and nloop > 0
    assert dec["slots"] == slots and int(desc.m) == host.shape[0] and int(desc.plan_bytes) == plan.nbytes == plan.buffer.numel(), what
    assert (dec["loopc"] is not None) == loops and (loops or int(desc.loop_offset) == -1), what
    assert info["loops_removed"] == (nloop if loops else 0), what
    built = {"forward": directions in ("both", "forward"), "transposed": directions in ("both", "transposed")}
    for t, (name, _) in enumerate(plan_buffer.DIRECTIONS):
        d = dec[name]
        if not built[name]:
            assert d is None and info["chunked_lists_" + name] == -1, (what, name)
            for field in ("off_", "dir_", "rec_", "entries_", "chunks_"):
                assert int(getattr(desc, field + name)) == -1, (what, field + name)
            continue
        tag = f"{what} {name}"
        lists = plan_buffer.expected_lists(host, p, n, G, drop, bool(t))
        want_len = np.zeros(slots, dtype=np.int64)
        for slot, l in lists.items():
            want_len[slot] = len(l)
        off = d["off"]
        assert off[0] == 0 and np.array_equal(np.diff(off), want_len), f"{tag}: off[]"
        assert off[slots] == d["entries"] == host.shape[0] - (nloop if drop else 0), f"{tag}: entries"
        want_ids = np.array([i for slot in sorted(lists) for _, i in lists[slot]], dtype=np.int32)
        assert np.array_equal(d["id"], want_ids), f"{tag}: the ids in list order"
        assert not d["zero"].any(), f"{tag}: zero words"
        want_dir = plan_buffer.expected_directory(lists, CHUNK)
        assert d["chunks"] == len(want_dir) and list(zip(d["dir_slot"].tolist(), d["dir_k"].tolist())) == want_dir, f"{tag}: the directory"
        assert info["chunked_lists_" + name] == sum(1 for l in lists.values() if len(l) > CHUNK), f"{tag}: long lists"
        if not kw.get("normalize", True):                                      # the weights as they are
            want_rows = np.array([r for slot in sorted(lists) for r, _ in lists[slot]], dtype=np.int64)
            want_c = host[want_rows, 2] if kw.get("weighted", False) else np.ones(len(want_rows))
            assert np.array_equal(d["c"].view(np.int64), np.ascontiguousarray(want_c).view(np.int64)), f"{tag}: coefficients"
    return plan, dec


@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_shuffled_elimination_results(ops, elim, o_v):
    sc, ptr, n = elim[o_v]
    rows = shuffled(sc, ptr, 9)
    for kw in (dict(), dict(weighted=True, normalize=False), dict(add_self_loops=False)):
        check_format(ops, rows, ptr, n, f"{o_v} {kw}", **kw)
    for directions in ("forward", "transposed"):
        one, _ = check_format(ops, rows, ptr, n, f"{o_v} {directions}", directions=directions, weighted=True)
        assert int(one.desc.flags) & (256 | 512) == (256 if directions == "forward" else 512)
    plan, dec = check_format(ops, rows, ptr, n + 37, f"{o_v} num_nodes + 37", weighted=True)
    for layer in range(6):                                                     # trailing ids: no record, loop coefficient exactly 1
        lo, hi = layer * (n + 37) + n, (layer + 1) * (n + 37)
        assert bool((dec["loopc"][lo:hi] == 1.0).all())
        assert dec["forward"]["off"][lo] == dec["forward"]["off"][hi] and dec["transposed"]["off"][lo] == dec["transposed"]["off"][hi]


def test_unweighted_coefficients_are_the_exact_ones(ops, elim):
    """Unweighted degrees are integers, so every formulation sums them exactly: the records hold (deg_i^-1/2 * 1) * deg_j^-1/2 with
    deg = in-degree + 1, evaluated from the left in float64 -- numpy's bits."""
    sc, ptr, n = elim["random"]
    rows = shuffled(sc, ptr, 3)
    plan, dec = check_format(ops, rows, ptr, n, "unweighted")
    host = rows.cpu().numpy()
    for s in range(len(ptr) - 1):
        part = host[ptr[s]:ptr[s + 1]]
        deg = np.bincount(part[:, 1].astype(np.int64), minlength=n).astype(np.float64) + 1.0
        dis = 1.0 / np.sqrt(deg)
        fwd = dec["forward"]
        lo, hi = fwd["off"][s * n], fwd["off"][(s + 1) * n]
        tgt = np.repeat(np.arange(n), np.diff(fwd["off"][s * n:(s + 1) * n + 1]))
        want = (dis[fwd["id"][lo:hi]] * 1.0) * dis[tgt]
        assert np.array_equal(fwd["c"][lo:hi].view(np.int64), want.view(np.int64)), f"segment {s}: coefficients"
        assert np.array_equal(dec["loopc"][s * n:(s + 1) * n].view(np.int64), ((dis * 1.0) * dis).view(np.int64)), f"segment {s}: loopc"


def test_comb_and_hand_made_lists(ops):
    rows, ptr, n = comb(4)
    for kw in (dict(), dict(add_self_loops=False), dict(weighted=True, normalize=False)):
        check_format(ops, rows, ptr, n, f"comb {kw}", **kw)
    hand = torch.tensor(HAND_A + HAND_B, dtype=torch.float64).cuda()
    for kw in (dict(), dict(add_self_loops=False), dict(weighted=True, normalize=False, fill_value=2.0)):
        plan, dec = check_format(ops, hand, [0, 11, 11, 15], 9, f"hand-made {kw}", **kw)
    assert dec["loopc"][2] == 5.0 and dec["loopc"][9 + 4] == 2.0 and dec["loopc"][18 + 1] == 9.0   # the last loop row's weight, else fill
    check_format(ops, torch.zeros((0, 3), dtype=torch.float64, device="cuda"), [0, 0, 0], 5, "m = 0")


def test_buffer_trimmed_to_a_storage_of_its_own(ops):
    """Eight loop rows on every id of a path, scattered: the records that stay are a fifth of the rows, so less than 3/4 of the
    bound is in use and the used bytes are copied into a storage of exactly that size."""
    from rlap_amd import _lib
    n, rs = 40, np.random.RandomState(9)
    rows = [[i, j, 0.5 + rs.rand()] for j in range(n) for i in (j - 1, j + 1) if 0 <= i < n]
    rows += [[j, j, 1.0 + k + rs.rand()] for j in range(n) for k in range(8)]
    rows = np.array(rows)
    rs.shuffle(rows)
    sc = torch.from_numpy(rows).cuda()
    m = len(rows)
    bound = ctypes.c_size_t()
    assert _lib.load().rlap_snapshot_plan_bytes(m, 1, 1, n, _lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE | _lib.GCN_WEIGHTED, ctypes.byref(bound)) == 0
    plan, dec = check_format(ops, sc, [0, m], n, "path with eight loop rows an id", weighted=True)
    assert 4 * plan.nbytes < 3 * bound.value, "a condition of this test: the branch that copies is the one taken"
    assert plan.buffer.untyped_storage().nbytes() == plan.nbytes == int(plan.desc.plan_bytes) and plan.buffer.storage_offset() == 0
    assert plan.info["loops_removed"] == 8 * n and plan.desc.entries_forward == 2 * (n - 1)
    x = torch.randn(n, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(0)).cuda()
    assert plan.propagate(x).shape == (1, n, 3) and bool(torch.isfinite(plan.propagate(x, transpose=True)).all())
