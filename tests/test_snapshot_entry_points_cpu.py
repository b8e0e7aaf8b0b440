"""The Python -> C mapping of the five snapshot entry points, without a GPU: the device is the CPU and the library a stub that
records each call with its arguments (tables and rows read through their addresses) and writes an info struct of its own."""
import ctypes

import pytest
import torch

from rlap_amd import _lib, ops
from util import StubLib, f64_at, i64_at, stub_ops

# positional arguments of the five exports (include/rlap_hip.h); the first eight are the same everywhere
HEAD = "h sc m ptr S node_ptr G n "
SIGS = {
    "rlap_snapshot_stats": HEAD + "weighted tol max_iter nodes lam iters conv info",
    "rlap_snapshot_ppr": HEAD + "alpha eps tol flags out cap out_ptr info",
    "rlap_snapshot_subgraph": HEAD + "nodes nodes_ptr nodes_len flags out out_ptr ids cap ids_ptr info",
    "rlap_snapshot_gcn_norm": HEAD + "flags fill src dst val cap eptr info",
    "rlap_snapshot_propagate": HEAD + "flags fill x F y info",
}
ARENA = 12345   # arena_bytes the stub reports


def put(addr, ctype, values):
    p = ctypes.cast(addr, ctypes.POINTER(ctype))
    for i, v in enumerate(values):
        p[i] = v


class SnapStub(StubLib):
    """`statuses`: what the next calls of an export return (then `status`); `ppr_rows`: the rows a PPR call keeps."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []
        self.ppr_rows = 3

    def export(self, name, a):
        m, S, G = a["m"], a["S"], a["G"]
        rec = {k: a[k] for k in ("m", "S", "G", "n")}
        rec["sc"] = None if a["sc"] is None else f64_at(a["sc"], 3 * min(m, 64))   # (the rows of the small inputs)
        rec["ptr"] = i64_at(a["ptr"], S + 1)
        rec["node_ptr"] = None if a["node_ptr"] is None else i64_at(a["node_ptr"], G + 1)
        for k in ("weighted", "tol", "max_iter", "alpha", "eps", "flags", "fill", "cap", "nodes_len", "F"):
            if k in a:
                rec[k] = a[k]
        if name == "rlap_snapshot_subgraph":
            rec["nodes"] = None if a["nodes"] is None else i64_at(a["nodes"], a["nodes_len"])
            rec["nodes_ptr"] = None if a["nodes_ptr"] is None else i64_at(a["nodes_ptr"], S + 1)
            rec["null"] = [k for k in ("out", "ids") if a[k] is None]
        if name == "rlap_snapshot_gcn_norm":
            rec["null"] = [k for k in ("src", "dst", "val") if a[k] is None]
        if name == "rlap_snapshot_ppr":
            rec["null"] = [k for k in ("out",) if a[k] is None]
        if name == "rlap_snapshot_propagate":
            rec["x"] = None if a["x"] is None else f64_at(a["x"], (S // G) * a["n"] * a["F"] if a["flags"] & _lib.SPMM_X_PER_LAYER else a["n"] * a["F"])
        self.calls.append((name, rec))
        status = self.statuses.pop(0) if self.statuses else self.status
        info = a["info"]._obj
        if name == "rlap_snapshot_ppr":
            info.rows_needed = self.ppr_rows   # (reported with RLAP_E_OUT_CAPACITY too)
        if status:
            return status
        info.host_syncs = 2
        if name == "rlap_snapshot_stats":
            info.small_segments, info.lanczos_steps = S, 7
            put(a["nodes"], ctypes.c_int64, [s + 1 for s in range(S)])
            put(a["lam"], ctypes.c_double, [0.5 * s for s in range(S)])
            put(a["iters"], ctypes.c_int32, [7] * S)
            put(a["conv"], ctypes.c_int32, [s % 2 for s in range(S)])
            return 0
        info.arena_bytes = ARENA
        if name == "rlap_snapshot_ppr":
            info.steps = 35
            rows = self.ppr_rows
            put(a["out"], ctypes.c_double, [float(v) for r in range(rows) for v in (r, r, 0.25)])
            put(a["out_ptr"], ctypes.c_int64, [0] + [rows] * S)
        elif name == "rlap_snapshot_subgraph":
            info.rows_kept, info.ids_written = min(m, 1), min(a["cap"], 2)
            put(a["out"] or 0, ctypes.c_double, [9.0, 8.0, 0.5][:3 * min(m, 1)])
            put(a["ids"] or 0, ctypes.c_int64, [4, 5][:min(a["cap"], 2)])
            put(a["out_ptr"], ctypes.c_int64, [0] + [min(m, 1)] * S)
            put(a["ids_ptr"], ctypes.c_int64, [0] + [min(a["cap"], 2)] * S)
        elif name == "rlap_snapshot_gcn_norm":
            info.entries = a["cap"]
            put(a["eptr"], ctypes.c_int64, [0] + [a["cap"]] * S)
        else:
            info.entries, info.blocks = m, 3
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, SnapStub())


def the_call(stub, k=0, of=1):
    calls = stub.exports()
    assert len(calls) == of, calls
    return calls[k]


# two segments over ids 0..3: rows [row, col, w]
SC = torch.tensor([[1, 0, 0.5], [0, 1, 0.5], [3, 2, 2.0], [2, 3, 2.0], [2, 2, 1.5]], dtype=torch.float64)
PTR = [0, 2, 5]
M, N = 5, 4
EMPTY = torch.zeros((0, 3), dtype=torch.float64)


def common(rec, m=M, S=2, G=1, n=N, node_ptr=None):
    assert (rec["m"], rec["S"], rec["G"], rec["n"]) == (m, S, G, n)
    assert rec["node_ptr"] == node_ptr
    if m:
        assert rec["sc"] == SC.reshape(-1).tolist() and rec["ptr"] == PTR
    else:
        assert rec["sc"] is None and rec["ptr"] == [0] * (S + 1)   # (no rows: NULL, not the address of an empty tensor)


def test_stats(lib):
    res = ops.snapshot_stats(SC, PTR, N)
    name, rec = the_call(lib)
    assert name == "rlap_snapshot_stats"
    common(rec)
    assert (rec["weighted"], rec["tol"], rec["max_iter"]) == (0, 1e-10, 1000)
    assert res["nodes"].tolist() == [1, 2] and res["rows"].tolist() == [2, 3] and res["lambda_max"].tolist() == [0.0, 0.5]
    assert res["iters"].tolist() == [7, 7] and res["converged"].tolist() == [False, True] and res["converged"].dtype == torch.bool
    assert ops.last_stats == {"small_segments": 2, "large_segments": 0, "lanczos_steps": 7, "large_steps": 0, "large_launches": 0,
                              "host_syncs": 2, "not_converged": 0}
    ops.snapshot_stats(SC.float(), torch.tensor(PTR, dtype=torch.int32), N, node_ptr=(0, 2, 4), weighted=True, tol=1e-6, max_iter=64)
    rec = the_call(lib, 1, 2)[1]
    common(rec, G=2, node_ptr=[0, 2, 4])
    assert (rec["weighted"], rec["tol"], rec["max_iter"]) == (1, 1e-6, 64)
    ops.snapshot_stats(EMPTY, [0, 0, 0], 7)
    common(the_call(lib, 2, 3)[1], m=0, n=7)


def test_host_checks_come_in_order_and_launch_nothing(lib):
    for kw, msg in [(dict(sc=SC[:, :2]), "sc: an"), (dict(num_nodes=-1), "num_nodes"), (dict(ptr=[0, 2, 4]), "ptr"),
                    (dict(node_ptr=[0, 1, 2, 4]), "node_ptr has 3 graphs"), (dict(tol=0.0), "tol"), (dict(max_iter=1025), "max_iter"),
                    (dict(num_nodes=-1, tol=0.0), "num_nodes"), (dict(ptr=[0, 2, 4], max_iter=0), "ptr"), (dict(tol=-1, max_iter=0), "tol")]:
        a = dict(sc=SC, ptr=PTR, num_nodes=N)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.snapshot_stats(a.pop("sc"), a.pop("ptr"), a.pop("num_nodes"), **a)
    for fn in (ops.snapshot_ppr, ops.snapshot_subgraph, ops.snapshot_gcn_norm):
        with pytest.raises(ValueError, match="ptr"):
            fn(SC, [0, 2, 4], N)
    with pytest.raises(ValueError, match="num_nodes"):
        ops.snapshot_propagate(SC, PTR, True, torch.zeros(4, 1))
    with pytest.raises(ValueError, match="num_nodes"):
        ops.ppr_diffusion(torch.zeros((2, 0), dtype=torch.int64), None, -2)
    assert lib.exports() == [] and ops.last_stats is None


@pytest.mark.parametrize("weighted,loop,norm", [(True, False, True), (False, True, False), (True, True, True), (False, False, False)])
def test_ppr_flags_and_first_capacity(lib, weighted, loop, norm):
    out, pptr = ops.snapshot_ppr(SC, PTR, N, alpha=0.3, eps=1e-3, tol=1e-8, weighted=weighted, add_self_loop=loop, normalize_out=norm)
    name, rec = the_call(lib)
    assert name == "rlap_snapshot_ppr"
    common(rec)
    assert (rec["alpha"], rec["eps"], rec["tol"]) == (0.3, 1e-3, 1e-8)
    assert rec["flags"] == (1 if weighted else 0) | (2 if loop else 0) | (4 if norm else 0)
    assert rec["cap"] == 2 * min(N, M) ** 2 and rec["null"] == []   # S min(n, m)^2 below the 2^22 rows of the first guess
    assert out.tolist() == [[0.0, 0.0, 0.25], [1.0, 1.0, 0.25], [2.0, 2.0, 0.25]] and pptr.tolist() == [0, 3, 3]
    assert ops.last_stats == {"steps": 35, "small_tiles": 0, "large_tiles": 0, "groups": 0, "launches": 0, "rows_needed": 3,
                              "arena_bytes": ARENA, "host_syncs": 2, "output_retries": 0, "first_cap": 32}


def test_ppr_capacity(lib):
    ops.snapshot_ppr(SC, PTR, N, node_ptr=[0, 2, 4])
    rec = the_call(lib)[1]
    common(rec, G=2, node_ptr=[0, 2, 4])
    assert rec["cap"] == 32 and rec["flags"] == 1 | 4
    lib.ppr_rows = 0
    out, pptr = ops.snapshot_ppr(EMPTY, [0, 0], 9)
    rec = the_call(lib, 1, 2)[1]
    common(rec, m=0, S=1, n=9)
    assert rec["cap"] == 0 and rec["null"] == ["out"] and tuple(out.shape) == (0, 3)
    big = torch.ones((1 << 19, 3), dtype=torch.float64)   # 16 m + 64 beyond 2^22, S min(n, m)^2 beyond that
    ops.snapshot_ppr(big, [0, 1 << 19], 1 << 12)
    assert the_call(lib, 2, 3)[1]["cap"] == 16 * (1 << 19) + 64
    ops.snapshot_ppr(big[:4096], [0, 4096], 1 << 12)
    assert the_call(lib, 3, 4)[1]["cap"] == 1 << 22


def test_ppr_retries_once_with_the_rows_needed(lib):
    lib.ppr_rows, lib.statuses = 40, [_lib.E_OUT_CAPACITY]
    out, _ = ops.snapshot_ppr(SC, PTR, N)
    caps = [c[1]["cap"] for c in lib.exports()]
    assert caps == [32, 40] and tuple(out.shape) == (40, 3)
    assert ops.last_stats["output_retries"] == 1 and ops.last_stats["first_cap"] == 32 and ops.last_stats["rows_needed"] == 40
    before = dict(ops.last_stats)
    lib.statuses = [_lib.E_OUT_CAPACITY, _lib.E_OUT_CAPACITY, 0]
    with pytest.raises(RuntimeError, match=r"rlap: status 13 \(status 13\)"):
        ops.snapshot_ppr(SC, PTR, N)
    assert len(lib.exports()) == 4 and ops.last_stats == before   # (one retry, not two)


def test_ppr_diffusion(lib):
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]])
    idx, w = ops.ppr_diffusion(ei, torch.tensor([2.0, 2.0, 3.0, 3.0]), 4, alpha=0.5, add_self_loop=True, normalize_out=False)
    name, rec = the_call(lib)
    assert name == "rlap_snapshot_ppr" and (rec["m"], rec["S"], rec["G"], rec["n"], rec["node_ptr"]) == (5, 1, 1, 4, None)
    assert rec["ptr"] == [0, 5] and rec["flags"] == 1 | 8 | 2 and rec["alpha"] == 0.5 and rec["cap"] == 16
    # grouped by column, the id without edges with a row (3, 3, 0) of its own
    assert rec["sc"] == [1.0, 0.0, 2.0, 0.0, 1.0, 2.0, 2.0, 1.0, 3.0, 1.0, 2.0, 3.0, 3.0, 3.0, 0.0]
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2]] and w.tolist() == [0.25] * 3


def test_subgraph_id_capacities(lib):
    out, optr, ids, iptr = ops.snapshot_subgraph(SC, PTR, N)   # no list: min(2 m, layers * n)
    name, rec = the_call(lib)
    assert name == "rlap_snapshot_subgraph"
    common(rec)
    assert (rec["nodes"], rec["nodes_ptr"], rec["nodes_len"], rec["flags"], rec["cap"], rec["null"]) == (None, None, 0, 0, 8, [])
    assert out.tolist() == [[9.0, 8.0, 0.5]] and optr.tolist() == [0, 1, 1] and ids.tolist() == [4, 5] and iptr.tolist() == [0, 2, 2]
    assert ops.last_stats == {"rows_kept": 1, "ids_written": 2, "arena_bytes": ARENA, "host_syncs": 2}
    ops.snapshot_subgraph(SC, PTR, 2, relabel=True)
    rec = the_call(lib, 1, 2)[1]
    assert (rec["cap"], rec["flags"], rec["n"]) == (4, 1, 2)
    ops.snapshot_subgraph(SC, PTR, N, nodes=[3, 1, 1], remove_self_loops=True)   # one list: a copy per layer
    rec = the_call(lib, 2, 3)[1]
    assert (rec["nodes"], rec["nodes_ptr"], rec["nodes_len"], rec["flags"], rec["cap"]) == ([3, 1, 1], None, 3, 2, 6)
    ops.snapshot_subgraph(SC, PTR, N, nodes=torch.tensor([3, 1, 1]), node_ptr=[0, 2, 4], relabel=True, remove_self_loops=True)
    rec = the_call(lib, 3, 4)[1]
    common(rec, G=2, node_ptr=[0, 2, 4])
    assert (rec["nodes"], rec["flags"], rec["cap"]) == ([3, 1, 1], 3, 3)     # (S // G = 1 layer)
    ops.snapshot_subgraph(SC, PTR, N, nodes=[0, 1, 2], nodes_ptr=[0, 2, 3])   # a list per segment: their total
    rec = the_call(lib, 4, 5)[1]
    assert (rec["nodes"], rec["nodes_ptr"], rec["nodes_len"], rec["cap"]) == ([0, 1, 2], [0, 2, 3], 3, 3)


def test_subgraph_empty_inputs(lib):
    out, optr, ids, iptr = ops.snapshot_subgraph(EMPTY, [0], 6)   # no segment at all
    rec = the_call(lib)[1]
    assert (rec["m"], rec["S"], rec["G"], rec["n"], rec["sc"], rec["ptr"]) == (0, 0, 1, 6, None, [0])
    assert rec["cap"] == 0 and rec["null"] == ["out", "ids"]
    assert tuple(out.shape) == (0, 3) and optr.tolist() == [0] and ids.numel() == 0 and iptr.tolist() == [0]
    ops.snapshot_subgraph(EMPTY, [0, 0], 6, nodes=[])   # an empty list is still a list
    rec = the_call(lib, 1, 2)[1]
    assert (rec["S"], rec["nodes"], rec["nodes_len"], rec["cap"], rec["null"]) == (1, [], 0, 0, ["out", "ids"])


@pytest.mark.parametrize("weighted,loops,norm,dtype", [(False, True, True, torch.float32), (True, False, True, torch.float64),
                                                        (True, True, False, torch.float32), (False, False, False, torch.float64)])
def test_gcn_norm(lib, weighted, loops, norm, dtype):
    ei, val, eptr = ops.snapshot_gcn_norm(SC, PTR, N, weighted=weighted, add_self_loops=loops, fill_value=2.0, normalize=norm, dtype=dtype)
    name, rec = the_call(lib)
    assert name == "rlap_snapshot_gcn_norm"
    common(rec)
    cap = M + (2 * N if loops else 0)   # m + (S // G) * n with loops, m without
    assert rec["flags"] == (1 if weighted else 0) | (2 if loops else 0) | (4 if norm else 0) | (8 if dtype == torch.float32 else 0)
    assert (rec["fill"], rec["cap"], rec["null"]) == (2.0, cap, [])
    assert tuple(ei.shape) == (2, cap) and ei.dtype == torch.int64 and tuple(val.shape) == (cap,) and val.dtype == dtype
    assert eptr.tolist() == [0, cap, cap]
    assert ops.last_stats == {"entries": cap, "loops_removed": 0, "arena_bytes": ARENA, "host_syncs": 2}
    ops.snapshot_gcn_norm(SC, PTR, N, [0, 2, 4], weighted, loops, 1.0, norm, dtype)
    rec = the_call(lib, 1, 2)[1]
    common(rec, G=2, node_ptr=[0, 2, 4])
    assert rec["cap"] == M + (N if loops else 0) and rec["fill"] == 1.0
    ops.snapshot_gcn_norm(EMPTY, [0, 0], 3, add_self_loops=loops)
    rec = the_call(lib, 2, 3)[1]
    common(rec, m=0, S=1, n=3)
    assert rec["cap"] == (3 if loops else 0) and rec["null"] == ([] if loops else ["src", "dst", "val"])


@pytest.mark.parametrize("transpose", [False, True])
def test_propagate(lib, transpose):
    x = torch.arange(8, dtype=torch.float64).reshape(4, 2)
    y = ops.snapshot_propagate(SC, PTR, N, x, weighted=True, fill_value=2.0, transpose=transpose)
    name, rec = the_call(lib)
    assert name == "rlap_snapshot_propagate"
    common(rec)
    assert rec["flags"] == 1 | 2 | 4 | (16 if transpose else 0) and (rec["fill"], rec["F"]) == (2.0, 2)
    assert rec["x"] == x.reshape(-1).tolist() and tuple(y.shape) == (2, 4, 2) and y.dtype == torch.float64
    assert ops.last_stats == {"entries": M, "blocks": 3, "chunked_lists": 0, "arena_bytes": ARENA, "host_syncs": 2}
    x3 = torch.arange(12, dtype=torch.float32).reshape(1, 4, 3)
    y = ops.snapshot_propagate(SC, PTR, N, x3, [0, 2, 4], False, False, 1.0, False, transpose)
    rec = the_call(lib, 1, 2)[1]
    common(rec, G=2, node_ptr=[0, 2, 4])
    assert rec["flags"] == 32 | 64 | (16 if transpose else 0) and rec["F"] == 3 and tuple(y.shape) == (1, 4, 3) and y.dtype == torch.float32
    xg = x.clone().requires_grad_(True)
    ops.snapshot_propagate(SC, PTR, N, xg, transpose=transpose).sum().backward()   # backward: one x per layer, the other product
    fwd, bwd = lib.exports()[2][1], lib.exports()[3][1]
    assert fwd["flags"] == 2 | 4 | (16 if transpose else 0) and bwd["flags"] == 2 | 4 | 64 | (0 if transpose else 16)
    assert bwd["x"] == [1.0] * 16 and tuple(xg.grad.shape) == (4, 2) and len(lib.exports()) == 4


CALLS = {
    "rlap_snapshot_stats": lambda: ops.snapshot_stats(SC, PTR, N),
    "rlap_snapshot_ppr": lambda: ops.snapshot_ppr(SC, PTR, N),
    "rlap_snapshot_subgraph": lambda: ops.snapshot_subgraph(SC, PTR, N),
    "rlap_snapshot_gcn_norm": lambda: ops.snapshot_gcn_norm(SC, PTR, N),
    "rlap_snapshot_propagate": lambda: ops.snapshot_propagate(SC, PTR, N, torch.ones(4, 1)),
}


@pytest.mark.parametrize("name", sorted(CALLS))
def test_one_regrow_on_a_short_arena(lib, name):
    lib.statuses, lib.ws_needed = [_lib.E_WORKSPACE], 1 << 20
    CALLS[name]()
    kinds = [c[0] for c in lib.calls if c[0] != "rlap_set_rng_mode"]
    assert kinds == ["rlap_set_workspace", name, "rlap_workspace_needed", "rlap_set_workspace", name]
    sizes = [c[1]["ws_bytes"] for c in lib.calls if c[0] == "rlap_set_workspace"]
    assert sizes[0] < (1 << 20) <= sizes[1]
    assert lib.exports()[0][1] == lib.exports()[1][1] and ops.last_stats is not None


@pytest.mark.parametrize("name", sorted(CALLS))
@pytest.mark.parametrize("status", [1, 2, 3, 12, 5])
def test_statuses_become_exceptions(lib, name, status):
    CALLS[name]()
    before = dict(ops.last_stats)
    lib.status = status
    value_error = status in (1, 2, 3) or (status == 12 and name != "rlap_snapshot_subgraph")
    msg = f"rlap: status {status}" + ("" if value_error else f" (status {status})")
    if name == "rlap_snapshot_ppr" and status == 3:
        msg += " (or a weight is <= 0)"
    with pytest.raises(ValueError if value_error else RuntimeError) as e:
        CALLS[name]()
    assert str(e.value) == msg
    assert len(lib.exports()) == 2 and ops.last_stats == before
