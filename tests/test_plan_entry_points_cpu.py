"""The Python -> C mapping of the propagation plans, without a GPU: the device is the CPU and the library a stub that records each
call with its arguments (tables, rows and features read through their addresses) and writes a descriptor and an info struct of its
own -- in the style of tests/test_snapshot_entry_points_cpu.py."""
import ctypes

import pytest
import torch

from rlap_amd import _lib, adapters, ops
from util import StubLib, f64_at, i64_at, stub_ops

SIGS = {
    "rlap_snapshot_plan_bytes": "m S G n flags bytes",
    "rlap_snapshot_plan_build": "h sc m ptr S node_ptr G n flags fill plan plan_bytes desc info",
    "rlap_snapshot_plan_propagate": "h plan desc flags x F y info",
    "rlap_snapshot_propagate": "h sc m ptr S node_ptr G n flags fill x F y info",
}
ARENA, BOUND, USED = 12345, 8192, 4096   # what the stub reports: arena bytes, the size query's bound, the bytes a build used


class PlanStub(StubLib):
    """`statuses`: what the next device calls return (then `status`)."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []
        self.used = USED

    def export(self, name, a):
        if name == "rlap_snapshot_plan_bytes":
            self.calls.append((name, {k: a[k] for k in ("m", "S", "G", "n", "flags")}))
            a["bytes"]._obj.value = BOUND
            return 0
        status = self.statuses.pop(0) if self.statuses else self.status
        info = a["info"]._obj
        if name == "rlap_snapshot_plan_build":
            m, S, G = a["m"], a["S"], a["G"]
            rec = {k: a[k] for k in ("m", "S", "G", "n", "flags", "fill", "plan_bytes")}
            rec["sc"] = None if a["sc"] is None else f64_at(a["sc"], 3 * m)
            rec["ptr"] = i64_at(a["ptr"], S + 1)
            rec["node_ptr"] = None if a["node_ptr"] is None else i64_at(a["node_ptr"], G + 1)
            rec["plan"] = a["plan"]
            self.calls.append((name, rec))
            d = a["desc"]._obj
            ctypes.memset(ctypes.addressof(d), 0, ctypes.sizeof(d))
            if status:
                return status
            d.m, d.segments, d.graphs, d.num_nodes, d.fill_value, d.flags, d.magic = m, S, G, a["n"], a["fill"], a["flags"], _lib.PLAN_MAGIC
            d.plan_bytes = self.used
            info.entries, info.blocks, info.arena_bytes, info.host_syncs = m + (S // G) * a["n"], 3, ARENA, 1
            info.chunked_lists_transposed = 0 if a["flags"] & _lib.PLAN_TRANSPOSED else -1
            info.chunked_lists_forward = 0 if a["flags"] & _lib.PLAN_FORWARD else -1
            return 0
        if name == "rlap_snapshot_propagate":
            self.calls.append((name, {"flags": a["flags"]}))
            return status
        d = a["desc"]._obj
        L, n, F = d.segments // d.graphs, d.num_nodes, a["F"]
        rec = {"plan": a["plan"], "flags": a["flags"], "F": F, "magic": d.magic, "desc_flags": d.flags, "null": [k for k in ("x", "y") if a[k] is None]}
        rec["x"] = None if a["x"] is None or a["flags"] & _lib.SPMM_X_F32 else f64_at(a["x"], L * n * F if a["flags"] & _lib.SPMM_X_PER_LAYER else n * F)
        self.calls.append((name, rec))
        if status:
            return status
        info.entries, info.arena_bytes, info.host_syncs = 99, ARENA, 0
        return 0

    def device_calls(self):
        return [c for c in self.exports() if c[0] != "rlap_snapshot_plan_bytes"]


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, PlanStub())


# two segments over ids 0..3: rows [row, col, w]
SC = torch.tensor([[1, 0, 0.5], [0, 1, 0.5], [3, 2, 2.0], [2, 3, 2.0], [2, 2, 1.5]], dtype=torch.float64)
PTR = [0, 2, 5]
M, N = 5, 4
EMPTY = torch.zeros((0, 3), dtype=torch.float64)
DIRS = {"forward": 256, "transposed": 512, "both": 768}


@pytest.mark.parametrize("directions", ["forward", "transposed", "both"])
@pytest.mark.parametrize("weighted,loops,norm", [(False, True, True), (True, False, True), (True, True, False), (False, False, False)])
def test_build_arguments(lib, weighted, loops, norm, directions):
    plan = ops.snapshot_plan(SC, PTR, N, weighted=weighted, add_self_loops=loops, fill_value=2.0, normalize=norm, directions=directions)
    (qname, q), (bname, b) = lib.exports()
    flags = (1 if weighted else 0) | (2 if loops else 0) | (4 if norm else 0) | DIRS[directions]
    assert qname == "rlap_snapshot_plan_bytes" and q == {"m": M, "S": 2, "G": 1, "n": N, "flags": flags}
    assert bname == "rlap_snapshot_plan_build" and (b["m"], b["S"], b["G"], b["n"], b["flags"], b["fill"]) == (M, 2, 1, N, flags, 2.0)
    assert b["sc"] == SC.reshape(-1).tolist() and b["ptr"] == PTR and b["node_ptr"] is None
    assert b["plan_bytes"] == BOUND and b["plan"]                             # the buffer is as large as the size query said
    assert isinstance(plan, ops.SnapshotPlan) and plan.buffer.dtype == torch.uint8 and plan.nbytes == USED   # trimmed to what is in use
    assert (plan.layers, plan.num_nodes, plan.entries, plan.directions) == (2, N, M + 2 * N, directions)
    assert ops.last_stats == {"entries": M + 2 * N, "blocks": 3, "chunked_lists_forward": 0 if flags & 256 else -1,
                              "chunked_lists_transposed": 0 if flags & 512 else -1, "loops_removed": 0, "arena_bytes": ARENA, "host_syncs": 1}


def test_build_with_node_ptr_and_without_rows(lib):
    plan = ops.snapshot_plan(SC.float(), torch.tensor(PTR, dtype=torch.int32), N, [0, 2, 4], True, True, 1.0, True, "forward")
    b = lib.device_calls()[0][1]
    assert (b["G"], b["node_ptr"], b["flags"], b["fill"]) == (2, [0, 2, 4], 1 | 2 | 4 | 256, 1.0) and plan.layers == 1
    assert lib.exports()[0][1]["G"] == 2
    lib.used = BOUND                                                          # nothing to trim: the buffer as allocated
    plan = ops.snapshot_plan(EMPTY, [0, 0, 0], 7)
    b = lib.device_calls()[1][1]
    assert (b["m"], b["sc"], b["ptr"], b["n"], b["flags"]) == (0, None, [0, 0, 0], 7, 2 | 4 | 768)   # no rows: NULL
    assert plan.nbytes == BOUND and plan.entries == 14 and plan.layers == 2


def test_host_checks_launch_nothing(lib):
    for kw, msg in [(dict(sc=SC[:, :2]), "sc: an"), (dict(num_nodes=-1), "num_nodes"), (dict(ptr=[0, 2, 4]), "ptr"),
                    (dict(node_ptr=[0, 1, 2, 4]), "node_ptr has 3 graphs"), (dict(fill_value=0.0), "fill_value"),
                    (dict(fill_value=float("inf")), "fill_value"), (dict(directions="backward"), "directions"),
                    (dict(directions=None), "directions"), (dict(ptr=[0]), "ptr")]:
        a = dict(sc=SC, ptr=PTR, num_nodes=N)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.snapshot_plan(a.pop("sc"), a.pop("ptr"), a.pop("num_nodes"), **a)
    assert lib.exports() == [] and ops.last_stats is None


@pytest.mark.parametrize("transpose", [False, True])
def test_planned_call_arguments(lib, transpose):
    lib.used = BOUND                                                          # (nothing trimmed: the buffer of the build is the plan's)
    plan = ops.snapshot_plan(SC, PTR, N, weighted=True)
    build = lib.device_calls()[0][1]
    x = torch.arange(8, dtype=torch.float64).reshape(4, 2)
    y = plan.propagate(x, transpose=transpose)
    name, rec = lib.device_calls()[1]
    assert name == "rlap_snapshot_plan_propagate" and rec["plan"] == plan.buffer.data_ptr() == build["plan"]
    assert (rec["flags"], rec["F"], rec["null"]) == (16 if transpose else 0, 2, [])
    assert (rec["magic"], rec["desc_flags"]) == (_lib.PLAN_MAGIC, 1 | 2 | 4 | 768)   # the descriptor the build wrote
    assert rec["x"] == x.reshape(-1).tolist() and tuple(y.shape) == (2, 4, 2) and y.dtype == torch.float64
    assert ops.last_stats == {"entries": 99, "blocks": 0, "chunked_lists": 0, "arena_bytes": ARENA, "host_syncs": 0}
    x3 = torch.arange(24, dtype=torch.float32).reshape(2, 4, 3)
    y = plan.propagate(x3, transpose)
    rec = lib.device_calls()[2][1]
    assert rec["flags"] == 32 | 64 | (16 if transpose else 0) and rec["F"] == 3 and tuple(y.shape) == (2, 4, 3) and y.dtype == torch.float32
    assert all(c[0] != "rlap_snapshot_propagate" for c in lib.exports())      # the unplanned export is not what serves a plan
    # backward: one x per layer, the other direction, the same plan
    xg = x.clone().requires_grad_(True)
    plan.propagate(xg, transpose=transpose).sum().backward()
    fwd, bwd = lib.device_calls()[3][1], lib.device_calls()[4][1]
    assert fwd["flags"] == (16 if transpose else 0) and bwd["flags"] == 64 | (0 if transpose else 16)
    assert bwd["x"] == [1.0] * 16 and bwd["plan"] == fwd["plan"] and tuple(xg.grad.shape) == (4, 2) and len(lib.device_calls()) == 5
    xg3 = torch.ones(2, 4, 2, dtype=torch.float64, requires_grad=True)
    plan.propagate(xg3, transpose=transpose).sum().backward()
    assert lib.device_calls()[6][1]["flags"] == 64 | (0 if transpose else 16) and tuple(xg3.grad.shape) == (2, 4, 2)


def test_empty_features_are_null(lib):
    plan = ops.snapshot_plan(EMPTY, [0, 0], 0)
    y = plan.propagate(torch.zeros(0, 4))
    rec = lib.device_calls()[1][1]
    assert rec["null"] == ["x", "y"] and rec["F"] == 4 and tuple(y.shape) == (1, 0, 4)


@pytest.mark.parametrize("directions,refused", [("forward", True), ("transposed", False)])
def test_a_missing_direction_raises_before_any_export(lib, directions, refused):
    plan = ops.snapshot_plan(SC, PTR, N, directions=directions)
    n0 = len(lib.exports())
    x = torch.ones(4, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match=directions):
        plan.propagate(x, transpose=refused)
    with pytest.raises(ValueError, match=directions):                         # the backward pass would need the other direction
        plan.propagate(x.clone().requires_grad_(True), transpose=not refused)
    with pytest.raises(ValueError, match="rows"):
        plan.propagate(torch.ones(5, 2), transpose=not refused)
    with pytest.raises(ValueError, match="layers"):
        plan.propagate(torch.ones(3, 4, 2), transpose=not refused)
    assert len(lib.exports()) == n0
    plan.propagate(x, transpose=not refused)                                  # the direction it holds
    with torch.no_grad():
        plan.propagate(x.clone().requires_grad_(True), transpose=not refused)
    assert len(lib.exports()) == n0 + 2


def test_one_regrow_on_a_short_arena(lib):
    lib.statuses, lib.ws_needed = [_lib.E_WORKSPACE], 1 << 20
    plan = ops.snapshot_plan(SC, PTR, N)
    kinds = [c[0] for c in lib.calls if c[0] != "rlap_set_rng_mode"]
    assert kinds == ["rlap_snapshot_plan_bytes", "rlap_set_workspace", "rlap_snapshot_plan_build", "rlap_workspace_needed", "rlap_set_workspace",
                     "rlap_snapshot_plan_build"]
    sizes = [c[1]["ws_bytes"] for c in lib.calls if c[0] == "rlap_set_workspace"]
    assert sizes[0] < (1 << 20) <= sizes[1]
    assert lib.device_calls()[0][1] == lib.device_calls()[1][1] and ops.last_stats["host_syncs"] == 1
    lib.calls.clear()
    lib.statuses, lib.ws_needed = [_lib.E_WORKSPACE], 1 << 22
    plan.propagate(torch.ones(4, 1))
    kinds = [c[0] for c in lib.calls if c[0] != "rlap_set_rng_mode"]
    assert kinds == ["rlap_snapshot_plan_propagate", "rlap_workspace_needed", "rlap_set_workspace", "rlap_snapshot_plan_propagate"]
    assert lib.calls[2][1]["ws_bytes"] >= 1 << 22 and ops.last_stats["host_syncs"] == 0


@pytest.mark.parametrize("which", ["build", "use"])
@pytest.mark.parametrize("status", [1, 2, 3, 12, 5])
def test_statuses_become_exceptions(lib, which, status):
    plan = ops.snapshot_plan(SC, PTR, N)
    if which == "use":
        plan.propagate(torch.ones(4, 1))
    before, n0 = dict(ops.last_stats), len(lib.device_calls())
    lib.status = status
    value_error = status in (1, 2, 3, 12)
    msg = f"rlap: status {status}" + ("" if value_error else f" (status {status})")
    with pytest.raises(ValueError if value_error else RuntimeError) as e:
        ops.snapshot_plan(SC, PTR, N) if which == "build" else plan.propagate(torch.ones(4, 1))
    assert str(e.value) == msg
    assert len(lib.device_calls()) == n0 + 1 and ops.last_stats == before


def test_snapshots_plan_builds_once_and_serves_the_conv(lib):
    snaps = adapters.Snapshots(SC, PTR, N, weighted=True, fill_value=2.0)
    planned = snaps.plan()
    assert isinstance(planned, adapters.PlannedSnapshots) and planned.layers == snaps.layers == 2 and planned.num_nodes == N
    assert lib.exports() == [] and planned.snapshot_plan is None              # built on first use
    with pytest.raises(ValueError, match="directions"):
        snaps.plan("sideways")
    torch.manual_seed(0)
    conv = adapters.SnapshotGCNConv(3, 2).double()
    x = torch.ones(4, 3, dtype=torch.float64, requires_grad=True)
    out = conv(x, planned)
    assert tuple(out.shape) == (2, 4, 2)
    out.sum().backward()
    kinds = [c[0] for c in lib.device_calls()]
    assert kinds == ["rlap_snapshot_plan_build", "rlap_snapshot_plan_propagate", "rlap_snapshot_plan_propagate"]
    b = lib.device_calls()[0][1]
    assert (b["flags"], b["fill"]) == (1 | 2 | 4 | 768, 2.0)                   # weighted, loops, normalised, both directions
    assert [c[1]["flags"] for c in lib.device_calls()[1:]] == [0, 16 | 64]
    planned.propagate(torch.ones(4, 1), transpose=True)
    assert [c[0] for c in lib.device_calls()].count("rlap_snapshot_plan_build") == 1
    one = snaps.plan("forward")
    with pytest.raises(ValueError, match="forward"):
        one.propagate(torch.ones(4, 1), transpose=True)
    snaps.propagate(torch.ones(4, 1))                                         # Snapshots.propagate itself: the unplanned call, as before
    assert lib.exports()[-1][0] == "rlap_snapshot_propagate"
