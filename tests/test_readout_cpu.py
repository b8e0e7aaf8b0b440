"""The per-graph readout (ops.graph_readout, rlap_graph_readout / _backward) without a GPU:

  * the rule -- spmm_mirror.list_sum(lib, ones, column) is the readout's definition (tests/csrc/spmm_mirror.cc around
    rlap_amd/csrc/rlap_spmm.h): against math.fsum within (n - 1) 2^-53 sum |x|, and bit for bit against a Python restatement of
    the chunk rule on both sides of the chunk edges;
  * the host-side arithmetic of rlap_amd/csrc/rlap_readout.h (clamped ranges, chunk counts, bounds, work item -> (graph, chunk), the
    dispatch rule of the launchers for every F) in a stand-alone program under -fsanitize=address,undefined, exhaustively for the tables of tests/test_gpu_readout.py and for
    tables that are not well formed;
  * the Python -> C mapping of both exports on a stub library, in the style of tests/test_plan_entry_points_cpu.py;
  * the layout of rlap_readout_info against _lib.ReadoutInfo;
  * the adapters of the graph-level step on stubs: node_ptr_of, the (K, G) table of rLapViews.snapshots(g, node_ptr=),
    Snapshots.aggregate / .readout, SnapshotGINConv, PlannedSnapshots.aggregate.
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import spmm_mirror
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, f64_at, i64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
CHUNK = 256


# ------------------------------------------------------------------------------------------------ the rule
@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    lib = spmm_mirror.build(tmp_path_factory.mktemp("spmm"))
    assert lib.spmm_chunk() == CHUNK
    return lib


def column(n, seed):
    rng = np.random.RandomState(seed)
    return rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-5.0, 5.0, size=n)


def chunk_rule(x):
    """The rule written out: chunks of CHUNK entries summed from 0 in order, the chunk sums added to 0 in chunk order."""
    total = np.float64(0.0)
    for b in range(0, len(x), CHUNK):
        c = np.float64(0.0)
        for v in x[b:b + CHUNK]:
            c = c + np.float64(1.0) * np.float64(v)
        total = total + c
    return total


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_the_rule_bit_for_bit(mirror, n):
    x = column(n, 100 + n)
    got = spmm_mirror.list_sum(mirror, np.ones(n), x)
    assert np.float64(got).tobytes() == np.float64(chunk_rule(x)).tobytes()
    if n == 0:
        assert got.tobytes() == np.float64(0.0).tobytes()        # an empty graph: exactly +0


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513, 1000, 2797])
def test_the_rule_against_fsum(mirror, n):
    x = column(n, 200 + n)
    got = float(spmm_mirror.list_sum(mirror, np.ones(n), x))
    assert abs(got - math.fsum(x)) <= (n - 1) * U * math.fsum(np.abs(x))


def test_a_negative_zero_sum_is_positive_zero(mirror):
    """0 + (-0) = +0: the chunk sums are added to 0, so a graph of -0.0 features reads out +0.0."""
    got = spmm_mirror.list_sum(mirror, np.ones(3), np.array([-0.0, -0.0, -0.0]))
    assert np.float64(got).tobytes() == np.float64(0.0).tobytes()


# ------------------------------------------------------------------------------------------------ the work map, under the sanitizers
SIZES_A = [0, 1, 255, 256, 257, 0, 512, 513, 1000, 3]
WELL_FORMED = [
    [0] + np.cumsum(SIZES_A).tolist(),
    [0, sum(SIZES_A)],
    [0] + np.cumsum(np.random.RandomState(3).randint(1, 41, size=300)).tolist(),
    [0, 2, 2, 5],
    [0, 0],
    [0, 0, 0, 0],
    [0, 256], [0, 257], [0, 256, 512, 768], [0, 257, 514], [0, 1, 2, 3, 4],
    [0] + np.cumsum([257] * 40).tolist(),                     # every graph is chunked: the arena's bound is met
]
MALFORMED = [   # (N, table): decreasing, beyond N, negative, not starting at 0
    (10, [0, 7, 3, 10]), (10, [0, 20]), (10, [0, 5, 20, 25]), (10, [-4, 3, 10]), (10, [3, 10]), (600, [0, 600, 0, 600, 0, 600]),
    (5, [9, 9, 9]), (300, [0, 300, 10, 290]),
]


def test_the_work_map_under_asan_ubsan(tmp_path):
    exe = tmp_path / "readout_map"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "readout_map_main.cc")])
    lines = [" ".join(map(str, [1, t[-1], len(t) - 1] + list(t))) for t in WELL_FORMED]
    lines += [" ".join(map(str, [0, N, len(t) - 1] + list(t))) for N, t in MALFORMED]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"{len(lines)} tables, 0 failures" in r.stdout
    # readout::dispatch over F = 1..65,536, two element sizes, two alignments: the cases, those of the narrow kernel (F <= 32, or 16
    # bytes a lane and F <= 32 V), those of 16 bytes a lane (aligned and F a multiple of V = 4, 2)
    assert f"dispatch {4 * 65536} {32 + 32 + (32 + 24) + (32 + 16)} {65536 // 4 + 65536 // 2}" in r.stdout.splitlines()
    got = [tuple(map(int, ln.split()[1:])) for ln in r.stdout.splitlines() if ln.startswith("table ")]
    for t, (chunks, chunked, part) in zip(WELL_FORMED, got):      # the counts ops.GraphTable reports are the header's
        sizes = np.diff(t)
        assert chunks == int(((sizes + CHUNK - 1) // CHUNK).sum()) and chunked == int((sizes > CHUNK).sum())
        assert part == int(((sizes + CHUNK - 1) // CHUNK)[sizes > CHUNK].sum())
        table = ops.GraphTable(t, t[-1])
        assert (table.chunks, table.chunked_graphs, table.graphs) == (chunks, chunked, len(t) - 1)


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_graph_readout": "h x L n F node_ptr G flags y info",
    "rlap_graph_readout_backward": "h gy L n F node_ptr G flags gx info",
    "rlap_snapshot_propagate": "h sc m ptr S node_ptr G n flags fill x F y info",
    "rlap_snapshot_plan_bytes": "m S G n flags bytes",
    "rlap_snapshot_plan_build": "h sc m ptr S node_ptr G n flags fill plan plan_bytes desc info",
    "rlap_snapshot_plan_propagate": "h plan desc flags x F y info",
}
ARENA = 4321


class ReadoutStub(StubLib):
    """Records every export; the readout writes the bound counts a library without the table would, and y = 1 (gx = 2)."""

    def __init__(self):
        super().__init__(SIGS)
        self.statuses = []

    def export(self, name, a):
        if name == "rlap_snapshot_plan_bytes":
            a["bytes"]._obj.value = 1024
            self.calls.append((name, {"flags": a["flags"]}))
            return 0
        status = self.statuses.pop(0) if self.statuses else self.status
        info = a["info"]._obj
        if name in ("rlap_graph_readout", "rlap_graph_readout_backward"):
            back = name.endswith("backward")
            src, dst = ("gy", "gx") if back else ("x", "y")
            L, n, F, G = a["L"], a["n"], a["F"], a["G"]
            rec = {k: a[k] for k in ("L", "n", "F", "G", "flags")}
            rec["node_ptr"] = i64_at(a["node_ptr"], G + 1)
            rec["node_ptr_addr"] = a["node_ptr"]
            rows_in, rows_out = (G, n) if back else (n, G)
            rec["null"] = [k for k in (src, dst) if a[k] is None]
            if a[src] is not None and not a["flags"] & _lib.READOUT_X_F32:
                rec["in"] = f64_at(a[src], L * rows_in * F)
            self.calls.append((name, rec))
            if status:
                return status
            if a[dst] is not None:
                ct = ctypes.c_float if a["flags"] & _lib.READOUT_X_F32 else ctypes.c_double
                out = ctypes.cast(a[dst], ctypes.POINTER(ct))
                for i in range(L * rows_out * F):
                    out[i] = 2.0 if back else 1.0
            info.rows, info.graphs, info.chunks, info.chunked_graphs = n, G, (n + 255) // 256 + G, min(G, n // 257)
            info.arena_bytes, info.host_syncs = ARENA, 0
            return 0
        if name == "rlap_snapshot_plan_build":
            d = a["desc"]._obj
            ctypes.memset(ctypes.addressof(d), 0, ctypes.sizeof(d))
            self.calls.append((name, {"flags": a["flags"], "G": a["G"], "fill": a["fill"]}))
            d.m, d.segments, d.graphs, d.num_nodes, d.flags, d.magic, d.plan_bytes = a["m"], a["S"], a["G"], a["n"], a["flags"], _lib.PLAN_MAGIC, 512
            info.entries = a["m"]
            return status
        self.calls.append((name, {"flags": a["flags"], "F": a["F"], "G": a.get("G"), "fill": a.get("fill")}))
        return status


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, ReadoutStub())


NODE_PTR = [0, 2, 2, 5]
N, G = 5, 3


def features(*shape, dtype=torch.float64):
    return (torch.arange(int(np.prod(shape)), dtype=torch.float64).reshape(shape) / 4.0 - 3.0).to(dtype)


@pytest.mark.parametrize("reduce,bit", [("sum", 0), ("mean", 1)])
@pytest.mark.parametrize("dtype,tbit", [(torch.float64, 0), (torch.float32, 32)])
def test_arguments_of_the_forward_export(lib, reduce, bit, dtype, tbit):
    x = features(2, N, 3, dtype=dtype)
    y = ops.graph_readout(x, NODE_PTR, reduce=reduce)
    (name, c), = lib.exports()
    assert name == "rlap_graph_readout"
    assert (c["L"], c["n"], c["F"], c["G"], c["flags"], c["node_ptr"], c["null"]) == (2, N, 3, G, bit | tbit, NODE_PTR, [])
    if dtype == torch.float64:
        assert c["in"] == x.reshape(-1).tolist()
    assert y.shape == (2, G, 3) and y.dtype == dtype and bool((y == 1).all())
    # last_stats: the library's report, with the counts this host knows exactly from its table
    assert ops.last_stats == {"rows": N, "graphs": G, "chunks": 2, "chunked_graphs": 0, "arena_bytes": ARENA, "host_syncs": 0}


def test_two_dimensional_features_are_one_layer(lib):
    x = features(N, 4)
    y = ops.graph_readout(x, torch.tensor(NODE_PTR, dtype=torch.int32), "mean")
    (_, c), = lib.exports()
    assert (c["L"], c["n"], c["F"], c["G"], c["flags"]) == (1, N, 4, G, 1) and c["in"] == x.reshape(-1).tolist()
    assert y.shape == (G, 4)


def test_no_rows_pass_null_pointers(lib):
    y = ops.graph_readout(torch.zeros(2, 0, 3), [0, 0, 0])
    (_, c), = lib.exports()
    assert (c["L"], c["n"], c["G"], c["null"], c["node_ptr"]) == (2, 0, 2, ["x"], [0, 0, 0]) and y.shape == (2, 2, 3)


def test_a_graph_table_is_checked_and_copied_once(lib):
    table = ops.GraphTable([0, 300, 300, 900], 900)
    assert (table.graphs, table.chunks, table.chunked_graphs) == (3, 2 + 3, 2)
    ops.graph_readout(torch.zeros(900, 1), table)
    ops.graph_readout(torch.zeros(2, 900, 2), table, "mean")
    a, b = lib.exports()
    assert a[1]["node_ptr_addr"] == b[1]["node_ptr_addr"] and a[1]["node_ptr"] == [0, 300, 300, 900]
    assert ops.last_stats["chunks"] == 5 and ops.last_stats["chunked_graphs"] == 2          # exact, not the stub's bounds
    with pytest.raises(ValueError):
        ops.graph_readout(torch.zeros(901, 1), table)


@pytest.mark.parametrize("x,node_ptr,reduce", [
    (torch.zeros(5), NODE_PTR, "sum"),                           # not 2-D or 3-D
    (torch.zeros(1, 2, 5, 3), NODE_PTR, "sum"),
    (torch.zeros(5, 3, dtype=torch.float16), NODE_PTR, "sum"),   # not float32 / float64
    (torch.zeros(5, 3, dtype=torch.int64), NODE_PTR, "sum"),
    (torch.zeros(5, 0), NODE_PTR, "sum"),                        # no column
    ([[1.0, 2.0]] * 5, NODE_PTR, "sum"),                         # not a tensor
    (torch.zeros(5, 3), [0, 2, 6], "sum"),                       # node_ptr[-1] != num_nodes
    (torch.zeros(5, 3), [0, 3, 2, 5], "sum"),                    # decreasing
    (torch.zeros(5, 3), [1, 5], "sum"),                          # does not start at 0
    (torch.zeros(5, 3), [5], "sum"),                             # no graph
    (torch.zeros(5, 3), [0.0, 5.0], "sum"),                      # not integers
    (torch.zeros(5, 3), [[0, 5]], "sum"),                        # not 1-D
    (torch.zeros(5, 3), NODE_PTR, "max"),                        # out of scope
    (torch.zeros(5, 3), NODE_PTR, None),
    (torch.zeros(5, 3), NODE_PTR, 1),
])
def test_bad_arguments_raise_value_error_before_any_call(lib, monkeypatch, x, node_ptr, reduce):
    def reached(*a, **k):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    with pytest.raises(ValueError):
        ops.graph_readout(x, node_ptr, reduce=reduce)
    assert lib.exports() == []


@pytest.mark.parametrize("status,exc", [(3, ValueError), (9, RuntimeError), (7, RuntimeError)])
def test_status_to_exception(lib, status, exc):
    lib.status = status
    before = ops.last_stats
    with pytest.raises(exc, match=f"status {status}"):
        ops.graph_readout(features(N, 2), NODE_PTR)
    assert ops.last_stats is before


def test_a_small_arena_is_grown_once(lib):
    lib.statuses = [_lib.E_WORKSPACE]
    lib.ws_needed = 1 << 20
    ops.graph_readout(features(N, 2), NODE_PTR)
    names = [c[0] for c in lib.calls]
    i = names.index("rlap_graph_readout")
    assert names[i:i + 4] == ["rlap_graph_readout", "rlap_workspace_needed", "rlap_set_workspace", "rlap_graph_readout"]
    assert lib.calls[i + 2][1]["ws_bytes"] >= 1 << 20


@pytest.mark.parametrize("reduce,bit", [("sum", 0), ("mean", 1)])
@pytest.mark.parametrize("shape", [(N, 3), (2, N, 3)])
@pytest.mark.parametrize("dtype,tbit", [(torch.float64, 0), (torch.float32, 32)])
def test_autograd_calls_the_backward_export(lib, reduce, bit, shape, dtype, tbit):
    x = features(*shape, dtype=dtype).requires_grad_(True)
    y = ops.graph_readout(x, NODE_PTR, reduce=reduce)
    gy = features(*y.shape, dtype=dtype) + 0.5
    y.backward(gy)
    (fname, f), (bname, b) = lib.exports()
    assert (fname, bname) == ("rlap_graph_readout", "rlap_graph_readout_backward")
    L = 1 if len(shape) == 2 else shape[0]
    assert (b["L"], b["n"], b["F"], b["G"], b["flags"], b["node_ptr"], b["null"]) == (L, N, 3, G, bit | tbit, NODE_PTR, [])
    assert b["flags"] == f["flags"] and b["node_ptr_addr"] == f["node_ptr_addr"]             # the same table, the same flags
    if dtype == torch.float64:
        assert b["in"] == gy.reshape(-1).tolist()
    assert x.grad.shape == x.shape and x.grad.dtype == dtype and bool((x.grad == 2).all())
    assert ops.last_stats["rows"] == N and ops.last_stats["host_syncs"] == 0


def test_no_graph_is_recorded_without_requires_grad(lib):
    assert not ops.graph_readout(features(N, 3), NODE_PTR).requires_grad
    x = features(N, 3).requires_grad_(True)
    with torch.no_grad():
        assert not ops.graph_readout(x, NODE_PTR).requires_grad


def test_readout_info_layout(tmp_path):
    """rlap_readout_info against _lib.ReadoutInfo, by the method of tests/test_cabi_symbols.py::test_layout_matches_the_header."""
    layout_matches_the_header(tmp_path, "rlap_readout_info", "ReadoutInfo")
    assert [f for f, _ in _lib.ReadoutInfo._fields_] == ["rows", "graphs", "chunks", "chunked_graphs", "arena_bytes", "host_syncs", "pad"]


def test_exports_and_flags_are_declared():
    assert {"rlap_graph_readout", "rlap_graph_readout_backward"} <= set(_lib.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "enum { RLAP_READOUT_MEAN = 1, RLAP_READOUT_X_F32 = 32 };" in hdr
    assert (_lib.READOUT_MEAN, _lib.READOUT_X_F32) == (1, 32)


# ------------------------------------------------------------------------------------------------ the adapters
def test_node_ptr_of():
    t = adapters.node_ptr_of(torch.tensor([0, 0, 1, 3, 3, 3]))
    assert t.tolist() == [0, 2, 3, 3, 6] and t.dtype == torch.int64 and t.device.type == "cpu"
    assert adapters.node_ptr_of(torch.tensor([0, 0, 1]), num_graphs=4).tolist() == [0, 2, 3, 3, 3]
    assert adapters.node_ptr_of(torch.tensor([], dtype=torch.int64), num_graphs=2).tolist() == [0, 0, 0]
    assert adapters.node_ptr_of(torch.tensor([], dtype=torch.int64)).tolist() == [0]
    assert adapters.node_ptr_of(torch.tensor([2, 2], dtype=torch.int32)).tolist() == [0, 0, 0, 2]
    for bad in (torch.tensor([0, 2, 1]), torch.tensor([1, 0]), torch.tensor([-1, 0]), torch.tensor([0.0, 1.0]), torch.tensor([[0, 1]])):
        with pytest.raises(ValueError):
            adapters.node_ptr_of(bad)
    with pytest.raises(ValueError):
        adapters.node_ptr_of(torch.tensor([0, 1, 2]), num_graphs=2)
    with pytest.raises(ValueError):
        adapters.node_ptr_of(torch.tensor([0, 1]), num_graphs=-1)


def two_paths():
    """Two path graphs, 0-1-2-3 and 4-5-6-7-8-9, as one batch."""
    a = torch.tensor([0, 1, 2, 4, 5, 6, 7, 8])
    return torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])]), [0, 4, 10]


@pytest.fixture
def eliminations(monkeypatch):
    seen = []

    def fake(name):
        def call(edge_index, edge_weights, num_nodes, num_remove, o_v, o_n, **kw):
            seen.append((name, num_nodes, num_remove, kw))
            S = len(kw["node_ptr"]) - 1
            S *= len(num_remove) * (kw.get("views", 1) if name == "depths" else 1)
            return torch.zeros((0, 3), dtype=torch.float64), torch.zeros(S + 1, dtype=torch.int64)
        return call
    monkeypatch.setattr(ops, "approximate_cholesky_views", fake("views"))
    monkeypatch.setattr(ops, "approximate_cholesky_depths", fake("depths"))
    return seen


def test_views_of_a_batch_remove_a_fraction_of_every_graph(eliminations):
    ei, node_ptr = two_paths()
    aug = adapters.rLapViews(fracs=(0.5, 0.3), o_v="degree", o_n="desc", keep_weights=True, seed=5, fill_value=2.0)
    x = torch.zeros(10, 3)
    s = aug.snapshots((x, ei, None), node_ptr=node_ptr)
    (name, n, num_remove, kw), = eliminations
    assert (name, n) == ("views", 10) and num_remove == [[2, 3], [1, 1]] == aug.num_remove          # int(frac * n_g), (K, G)
    assert kw["node_ptr"].tolist() == node_ptr and kw["seed"] == 5 and kw["return_device"] == "same"
    assert isinstance(s, adapters.Snapshots) and s.node_ptr.tolist() == node_ptr and s.num_nodes == 10 and s.layers == 2
    assert (s.weighted, s.fill_value) == (True, 2.0)
    assert "graph_shared.py" in adapters.rLapViews.snapshots.__doc__ and "graph_shared.py" in adapters.rLapDepths.snapshots.__doc__
    with pytest.raises(ValueError):
        aug.snapshots((torch.zeros(9, 3), ei, None), node_ptr=node_ptr)     # x and the batch disagree
    with pytest.raises(ValueError):
        aug.snapshots((x, ei, None), node_ptr=[0, 7, 4, 10])


def test_depths_of_a_batch(eliminations):
    ei, node_ptr = two_paths()
    aug = adapters.rLapDepths(fracs=(0.25, 0.5), views=2, seed=1)
    s = aug.snapshots((None, ei, None), node_ptr=torch.tensor(node_ptr))
    (name, n, num_remove, kw), = eliminations
    assert (name, n, kw["views"]) == ("depths", 10, 2) and num_remove == [[[1, 1], [1, 1]], [[2, 3], [2, 3]]]   # (D, R, G): int(frac * n_g)
    assert s.layers == 4 and s.node_ptr.tolist() == node_ptr


def test_without_node_ptr_nothing_changes(monkeypatch):
    ei, _ = two_paths()
    seen = []
    monkeypatch.setattr(ops, "approximate_cholesky_views",
                        lambda *a, **kw: seen.append((a[2], a[3], kw)) or (torch.zeros((0, 3), dtype=torch.float64), torch.zeros(3, dtype=torch.int64)))
    s = adapters.rLapViews(fracs=(0.5, 0.5)).snapshots((None, ei, None))
    assert seen[0][0] == 10 and seen[0][1] == [5, 5] and "node_ptr" not in seen[0][2] and s.node_ptr is None


SC = torch.tensor([[1, 0, 0.5], [0, 1, 0.5], [3, 2, 2.0], [2, 3, 2.0]], dtype=torch.float64)


@pytest.mark.parametrize("weighted", [False, True])
def test_aggregate_is_the_plain_neighbour_sum(lib, weighted):
    s = adapters.Snapshots(SC, [0, 2, 4], 4, [0, 2, 4], weighted, 3.0)
    s.aggregate(features(4, 2))
    s.aggregate(features(1, 4, 2, dtype=torch.float32), transpose=True)
    s.propagate(features(4, 2))
    a, b, c = lib.exports()
    w = _lib.GCN_WEIGHTED if weighted else 0
    assert a[0] == "rlap_snapshot_propagate" and a[1]["flags"] == w and a[1]["G"] == 2                      # no loops, no normalisation
    assert b[1]["flags"] == w | _lib.SPMM_TRANSPOSE | _lib.SPMM_X_F32 | _lib.SPMM_X_PER_LAYER
    assert c[1]["flags"] == w | _lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE                                    # propagate is as it was


def test_holder_readout_keeps_one_table(lib):
    s = adapters.Snapshots(SC, [0, 2, 4], 4, [0, 2, 4])
    y = s.readout(features(1, 4, 2))
    s.readout(features(4, 3), reduce="mean")
    s.plan().readout(features(4, 1))
    a, b, c = lib.exports()
    assert [t[0] for t in (a, b, c)] == ["rlap_graph_readout"] * 3 and y.shape == (1, 2, 2)
    assert a[1]["node_ptr"] == [0, 2, 4] and a[1]["node_ptr_addr"] == b[1]["node_ptr_addr"] == c[1]["node_ptr_addr"]
    assert (a[1]["flags"], b[1]["flags"], b[1]["L"]) == (0, 1, 1)
    one = adapters.Snapshots(SC, [0, 4], 4)                       # no node_ptr: the whole id range is one graph
    assert one.readout(torch.zeros(4, 2)).shape == (1, 2) and lib.exports()[-1][1]["node_ptr"] == [0, 4]


def test_planned_aggregate_builds_its_second_plan_once(lib):
    p = adapters.Snapshots(SC, [0, 2, 4], 4, [0, 2, 4], True, 1.0).plan()
    assert p.aggregate_plan is None
    for _ in range(3):
        p.aggregate(torch.zeros(4, 2))
    builds = [c for c in lib.exports() if c[0] == "rlap_snapshot_plan_build"]
    uses = [c for c in lib.exports() if c[0] == "rlap_snapshot_plan_propagate"]
    assert len(builds) == 1 and len(uses) == 3 and p.snapshot_plan is None and p.aggregate_plan is not None
    assert builds[0][1]["flags"] == _lib.GCN_WEIGHTED | _lib.PLAN_FORWARD | _lib.PLAN_TRANSPOSED and builds[0][1]["G"] == 2
    p.propagate(torch.zeros(4, 2))                                # the first plan is another one, with loops and the normalisation
    builds = [c for c in lib.exports() if c[0] == "rlap_snapshot_plan_build"]
    assert len(builds) == 2 and builds[1][1]["flags"] & (_lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE) == _lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE


class FakeSnapshots:
    """What SnapshotGINConv needs of a holder: aggregate(x) -> (L, n, F)."""
    layers = 2

    def aggregate(self, x):
        x3 = x if x.dim() == 3 else x.unsqueeze(0).expand(self.layers, *x.shape)
        return x3.flip(1) * torch.tensor([1.0, 2.0]).reshape(2, 1, 1)


def test_gin_conv_shapes_and_eps():
    torch.manual_seed(0)
    conv = adapters.SnapshotGINConv(torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.ReLU(), torch.nn.Linear(5, 4)), eps=0.5, train_eps=True)
    assert isinstance(conv.eps, torch.nn.Parameter) and float(conv.eps.detach()) == 0.5 and "eps" in dict(conv.named_parameters())
    s = FakeSnapshots()
    x = torch.randn(6, 3, requires_grad=True)
    y = conv(x, s)
    assert y.shape == (2, 6, 4)
    want = conv.nn(1.5 * x + s.aggregate(x))
    assert torch.equal(y, want)
    z = conv.nn[0].weight.new_zeros(2, 6, 3).normal_()
    assert conv(z, s).shape == (2, 6, 4)                           # (L, n, F) features, one matrix per layer
    y.sum().backward()
    assert conv.eps.grad is not None and x.grad is not None and conv.nn[0].weight.grad is not None
    fixed = adapters.SnapshotGINConv(torch.nn.Identity())
    assert "eps" not in dict(fixed.named_parameters()) and float(fixed.eps) == 0.0 and "eps" in dict(fixed.named_buffers())
    assert torch.equal(fixed(x, s), x + s.aggregate(x))
    assert "PyG is not installed" in adapters.SnapshotGINConv.__doc__
