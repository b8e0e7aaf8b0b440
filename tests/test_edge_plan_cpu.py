"""Edge plans without a GPU (rlap_edge_plan_build, ops.edge_list_plan / edge_plan).

1. The degree rule of rlap_amd/csrc/rlap_edgeplan.h -- compiled here with g++ through tests/csrc/edgeplan_mirror.cc, the same
   functions rlap_edgeplan.hip's kernels read -- against a numpy restatement written from the prose of the issue alone: sequential
   float64 scalar adds, nothing imported from the header.  Degrees, dis, coefficients and loopc bit for bit.
2. Layout equivalence: on CPU-oracle elimination results the mirror's plan equals the tests/csrc/plan_mirror.cc construction (the
   layout of rlap_snapshot_plan_build) bit for bit, both directions; after a seeded shuffle inside every segment it equals a plain
   Python construction (tests/plan_buffer.py), and the product through tests/csrc/spmm_mirror.cc lies within (16 + 4 L) 2^-53 A of
   the float64 index_add_ reference of tests/test_gpu_propagate.py (its derivation is there).
3. The mirror as a stand-alone program under -fsanitize=address,undefined, malformed inputs included.
4. The Python -> C mapping of ops.edge_list_plan / ops.edge_plan / adapters.graph_plan / rLapDepths.diffuse_plan on a stub library,
   every ValueError raised before the device is touched, and the export's place in the header, _lib.EXPORTS and the checked call path.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import edgeplan_mirror
import plan_buffer
import spmm_mirror
from test_gpu_propagate import assert_close, bound_factor, yardstick
from util import StubLib, ba_graph, canonical, f64_at, i64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "rlap_amd", "csrc")
DEGREES = (0, 1, 15, 16, 17, 63, 64, 65, 129)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    d = tmp_path_factory.mktemp("edgeplan")
    so = os.path.join(str(d), "libplan_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", INC, "-o", so,
                           os.path.join(ROOT, "tests", "csrc", "plan_mirror.cc")])
    pm = ctypes.CDLL(so)
    i64, ci, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    pm.plan_dir_cap.restype = i64
    pm.plan_dir_cap.argtypes = [i64]
    pm.plan_build.restype = i64
    pm.plan_build.argtypes = [i64, vp, i64, vp, i64, i64, vp, ci, ci, vp, vp, vp, vp, vp, vp]
    return edgeplan_mirror.build(d), pm, spmm_mirror.build(d)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------ 1. the degree rule
def numpy_degree(ws, is_loop, loops, fill):
    """The prose of the rule: place k (loop rows counted) goes to lane k % 16, accumulator (k / 16) % 4, ascending k; a loop row adds
    nothing when loops are on; per lane (a0 + a1) + (a2 + a3); xor butterfly over 8, 4, 2, 1 lanes; the loop's weight -- the last
    loop row's, or fill -- last.  Returns (deg, loop weight)."""
    acc = [[np.float64(0.0)] * 4 for _ in range(16)]
    lw = np.float64(fill)
    for k, (w, lp) in enumerate(zip(ws, is_loop)):
        if loops and lp:
            lw = np.float64(w)
            continue
        acc[k % 16][(k // 16) % 4] = acc[k % 16][(k // 16) % 4] + np.float64(w)
    v = [(a[0] + a[1]) + (a[2] + a[3]) for a in acc]
    for o in (8, 4, 2, 1):
        v = [v[l] + v[l ^ o] for l in range(16)]
    return (v[0] + lw if loops else v[0]), lw


def numpy_dis(deg):
    return np.float64(1.0) / np.sqrt(np.float64(deg)) if deg > 0 else np.float64(0.0)


def numpy_plan_numbers(rows, ptr, N, G, weighted, loops, fill, normalize):
    """deg, dis, lw, loopc per slot and the coefficient of every row, from the lists in input order."""
    rows = np.asarray(rows, dtype=np.float64)
    slots = ((len(ptr) - 1) // G) * N
    lists = plan_buffer.expected_lists(rows, ptr, N, G, False, False)          # the target's list, loop rows counted
    deg, dis, lw = np.zeros(slots), np.zeros(slots), np.zeros(slots)
    for slot in range(slots):
        rs = [r for r, _ in lists.get(slot, [])]
        ws = [rows[r, 2] if weighted else 1.0 for r in rs]
        deg[slot], lw[slot] = numpy_degree(ws, [rows[r, 0] == rows[r, 1] for r in rs], loops, fill)
        dis[slot] = numpy_dis(deg[slot])
    loopc = np.array([(dis[s] * lw[s]) * dis[s] if normalize else lw[s] for s in range(slots)])
    c = np.zeros(rows.shape[0])
    for s in range(len(ptr) - 1):
        for r in range(ptr[s], ptr[s + 1]):
            w = np.float64(rows[r, 2] if weighted else 1.0)
            i, j = (s // G) * N + int(rows[r, 0]), (s // G) * N + int(rows[r, 1])
            c[r] = (dis[i] * w) * dis[j] if normalize else w
    return deg, dis, lw, loopc, c


def comb(with_loops, seed):
    """Targets 0..8 with in-degrees DEGREES, their sources ids 9.. (source k has out-degree = the number of targets of degree > k);
    with_loops: up to three loop rows per target at seeded places of its list.  Rows shuffled."""
    rs = np.random.RandomState(seed)
    rows = []
    for j, d in enumerate(DEGREES):
        rows += [[9 + k, j, 0.25 + rs.rand() * 10.0 ** rs.randint(-3, 4)] for k in range(d)]
        if with_loops:
            rows += [[j, j, 0.5 + rs.rand()] for _ in range(j % 4)]
    rows = np.array(rows, dtype=np.float64)
    rs.shuffle(rows)
    return rows, [0, len(rows)], 9 + max(DEGREES)


@pytest.mark.parametrize("with_loops", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
def test_degree_rule_against_numpy(libs, weighted, with_loops):
    ep = libs[0]
    assert ep.edgeplan_lanes() == 16 and ep.edgeplan_accs() == 4 and ep.edgeplan_places_consistent(1000) == 1
    assert [ep.edgeplan_key_bits(s) for s in (0, 1, 2, 3, 1024, 1025, (1 << 31) - 1)] == [1, 1, 1, 2, 10, 11, 31]
    rows, ptr, N = comb(with_loops, 5)
    for loops in (True, False):
        for normalize in (True, False):
            tag = f"weighted={weighted} loop rows={with_loops} loops={loops} normalize={normalize}"
            got = edgeplan_mirror.plan(ep, rows, ptr, N, weighted=weighted, add_self_loops=loops, fill_value=2.0, normalize=normalize)
            deg, dis, lw, loopc, c = numpy_plan_numbers(rows, ptr, N, 1, weighted, loops, 2.0, normalize)
            assert np.array_equal(bits(got["deg"]), bits(deg)), f"{tag}: degrees"
            assert np.array_equal(bits(got["dis"]), bits(dis)) and np.array_equal(bits(got["lw"]), bits(lw)), f"{tag}: dis / loop weights"
            if loops:
                assert np.array_equal(bits(got["loopc"]), bits(loopc)), f"{tag}: loopc"
            else:
                assert got["loopc"] is None
            drop = loops and with_loops
            for t, name in enumerate(("forward", "transposed")):
                order = plan_buffer.expected_lists(rows, ptr, N, 1, drop, bool(t))
                want = np.array([c[r] for slot in sorted(order) for r, _ in order[slot]])
                assert np.array_equal(bits(got[name]["c"]), bits(want)), f"{tag} {name}: coefficients"
            assert got["loops_removed"] == (int((rows[:, 0] == rows[:, 1]).sum()) if loops else 0)
    # the in-degrees the lanes meet: none, one lane, a full lane row, the accumulator wrap at 64, a second turn
    assert np.bincount(rows[rows[:, 0] != rows[:, 1], 1].astype(int), minlength=9)[:9].tolist() == list(DEGREES)
    if not weighted and not with_loops:
        assert got["deg"][:9].tolist() == [float(d) for d in DEGREES]           # (the last pass: loops off)
    out_deg = np.bincount(rows[rows[:, 0] != rows[:, 1], 0].astype(int), minlength=N)[9:]
    assert out_deg[0] == 8 and out_deg[-1] == 1


# ------------------------------------------------------------------------------------------------ 2. layout equivalence
def oracle_result(o_v):
    """BA(300, 3): two depths x two views, every segment one oracle elimination in the elimination layout (grouped by column)."""
    import oracle as pyoracle
    n = 300
    ei = ba_graph(n, 3, 2)
    parts = [canonical(pyoracle.approximate_cholesky(ei, None, n, t, o_v, "asc", shuffle_seed=seed,
                                                     perm=np.random.RandomState(seed).permutation(n) if o_v == "random" else None))
             for t in (75, 150) for seed in (3, 4)]
    ptr = [0] + [int(v) for v in np.cumsum([len(p) for p in parts])]
    return np.concatenate(parts), ptr, n


def mirror_of_snapshot_plan(pm, rows, ptr, N, c, drop):
    out = {"slots": (len(ptr) - 1) * N, "spans": []}
    m, S = rows.shape[0], len(ptr) - 1
    p = np.array(ptr, dtype=np.int64)
    for t, name in enumerate(("forward", "transposed")):
        cap = pm.plan_dir_cap(m)
        off = np.full(out["slots"] + 1, -7, dtype=np.int64)
        rec_c, rec_id = np.full(m, np.nan), np.full(m, -7, dtype=np.int32)
        dslot, dk = np.full(cap, -7, dtype=np.int64), np.full(cap, -7, dtype=np.int64)
        chunks = ctypes.c_int64(-1)
        ent = pm.plan_build(m, rows.ctypes.data, S, p.ctypes.data, 1, N, c.ctypes.data, int(drop), t, off.ctypes.data, rec_c.ctypes.data,
                            rec_id.ctypes.data, dslot.ctypes.data, dk.ctypes.data, ctypes.byref(chunks))
        assert ent >= 0
        out[name] = {"entries": int(ent), "chunks": chunks.value, "off": off, "c": rec_c[:ent], "id": rec_id[:ent],
                     "zero": np.zeros(ent, dtype=np.int32), "dir_slot": dslot[:chunks.value], "dir_k": dk[:chunks.value]}
    return out


def shuffled(rows, ptr, seed):
    rs = np.random.RandomState(seed)
    out = rows.copy()
    for s in range(len(ptr) - 1):
        out[ptr[s]:ptr[s + 1]] = rows[ptr[s]:ptr[s + 1]][rs.permutation(ptr[s + 1] - ptr[s])]
    return out


def check_python_construction(dec, rows, ptr, N, G, loops, chunk, what):
    """Lists, ids in order, off[], the directory and the zero words against tests/plan_buffer.py's plain construction."""
    drop = loops and bool((rows[:, 0] == rows[:, 1]).any())
    for t, name in enumerate(("forward", "transposed")):
        d = dec[name]
        lists = plan_buffer.expected_lists(rows, ptr, N, G, drop, bool(t))
        want_len = np.zeros(dec["slots"], dtype=np.int64)
        for slot, l in lists.items():
            want_len[slot] = len(l)
        assert d["off"][0] == 0 and np.array_equal(np.diff(d["off"]), want_len), f"{what} {name}: off[]"
        want_ids = np.array([i for slot in sorted(lists) for _, i in lists[slot]], dtype=np.int32)
        assert np.array_equal(d["id"], want_ids), f"{what} {name}: the ids in order"
        want_dir = plan_buffer.expected_directory(lists, chunk)
        assert list(zip(d["dir_slot"].tolist(), d["dir_k"].tolist())) == want_dir and d["chunks"] == len(want_dir), f"{what} {name}: directory"
        assert not d["zero"].any() and d["entries"] == len(want_ids)


def product_within_bound(sp, dec, rows, ptr, N, what, **kw):
    x = torch.from_numpy(np.random.RandomState(1).randn(N, 3))
    sc = torch.from_numpy(rows)
    for t, name in enumerate(("forward", "transposed")):
        ref, A, count, longest = yardstick(sc, ptr, N, x, transpose=bool(t), **kw)
        y = np.stack([spmm_mirror.entries(sp, src, dst, val, N, x.numpy(), False, bool(t))
                      for src, dst, val in edgeplan_mirror.entry_lists(dec, name, N)])
        assert_close(torch.from_numpy(y), ref, A, count, bound_factor(longest, True), f"{what} {name}")


@pytest.mark.parametrize("o_v", ["random", "degree", "coarsen"])
def test_layout_equivalence_on_oracle_results(libs, o_v):
    ep, pm, sp = libs
    rows, ptr, N = oracle_result(o_v)
    assert len(ptr) == 5 and rows.shape[0] > 0
    for weighted in (False, True):
        tag = f"{o_v} weighted={weighted}"
        _, _, _, loopc, c = numpy_plan_numbers(rows, ptr, N, 1, weighted, True, 1.0, True)
        got = edgeplan_mirror.plan(ep, rows, ptr, N, weighted=weighted)
        want = mirror_of_snapshot_plan(pm, rows, ptr, N, c, False)
        want["loopc"] = loopc
        assert plan_buffer.same_decoded(got, want), f"{tag}: differs from the plan_mirror.cc construction"
        mixed = shuffled(rows, ptr, 17)
        dec = edgeplan_mirror.plan(ep, mixed, ptr, N, weighted=weighted)
        check_python_construction(dec, mixed, ptr, N, 1, True, sp.spmm_chunk(), tag)
        product_within_bound(sp, dec, mixed, ptr, N, tag, weighted=weighted)


# ------------------------------------------------------------------------------------------------ 3. the sanitizer program
def test_the_mirror_under_asan_and_ubsan(tmp_path):
    """The mirror as a stand-alone program with its own main: a plain executable, nothing preloaded.  Its last inputs are malformed
    (an id out of range, an id 1.5, a ptr past m, an id of another graph of the batch): it reports the refusal and exits clean."""
    exe = tmp_path / "edgeplan_mirror_san"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-DEDGEPLAN_MIRROR_MAIN", "-Wall", "-Werror", "-I", INC, "-o", str(exe), edgeplan_mirror.SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": ok (0)") == 8 * 16 and "FAILED" not in r.stdout
    assert r.stdout.count("refused as expected") == 4 * 16 and "ptr past m flags 0 transpose 0: ok (0) refused" in r.stdout


# ------------------------------------------------------------------------------------------------ 4. the entry points
SIGS = {
    "rlap_snapshot_plan_bytes": "m S G n flags bytes",
    "rlap_edge_plan_build": "h sc m ptr S node_ptr G n flags fill plan plan_bytes desc info",
    "rlap_snapshot_plan_build": "h sc m ptr S node_ptr G n flags fill plan plan_bytes desc info",
    "rlap_snapshot_plan_propagate": "h plan desc flags x F y info",
    "rlap_snapshot_ppr": "h sc m ptr S node_ptr G n alpha eps tol flags out cap out_ptr info",
    "rlap_approx_chol_depths": "h row col w E n K num_remove o_v o_n perm seed out cap out_ptr stats",
}
ARENA, BOUND, USED = 777, 8192, 4096


class EdgeStub(StubLib):
    def __init__(self):
        super().__init__(SIGS)
        from rlap_amd import _lib
        self._lib = _lib
        self.used = USED

    def export(self, name, a):
        if name == "rlap_snapshot_plan_bytes":
            self.calls.append((name, {k: a[k] for k in ("m", "S", "G", "n", "flags")}))
            a["bytes"]._obj.value = BOUND
            return 0
        if name == "rlap_edge_plan_build":
            m, S, G = a["m"], a["S"], a["G"]
            rec = {k: a[k] for k in ("m", "S", "G", "n", "flags", "fill", "plan_bytes")}
            rec["sc"] = None if a["sc"] is None else f64_at(a["sc"], 3 * m)
            rec["ptr"] = i64_at(a["ptr"], S + 1)
            rec["node_ptr"] = None if a["node_ptr"] is None else i64_at(a["node_ptr"], G + 1)
            self.calls.append((name, rec))
            d = a["desc"]._obj
            ctypes.memset(ctypes.addressof(d), 0, ctypes.sizeof(d))
            if self.status:
                return self.status
            d.m, d.segments, d.graphs, d.num_nodes, d.fill_value, d.flags, d.magic = m, S, G, a["n"], a["fill"], a["flags"], self._lib.PLAN_MAGIC
            d.plan_bytes = self.used
            info = a["info"]._obj
            info.entries, info.blocks, info.arena_bytes, info.host_syncs = m + (S // G) * a["n"], 2, ARENA, 1
            return 0
        if name == "rlap_snapshot_plan_propagate":
            self.calls.append((name, {"flags": a["flags"], "F": a["F"]}))
            return self.status
        self.calls.append((name, {}))
        return 5


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, EdgeStub())


ROWS = torch.tensor([[2, 0, 0.5], [0, 1, 0.5], [2, 2, 2.0], [0, 1, 0.25], [3, 2, 1.5]], dtype=torch.float64)   # any order, a duplicate, a loop
DIRS = {"forward": 256, "transposed": 512, "both": 768}


@pytest.mark.parametrize("directions", ["forward", "transposed", "both"])
@pytest.mark.parametrize("weighted,loops,norm", [(False, True, True), (True, False, True), (True, True, False), (False, False, False)])
def test_edge_list_plan_arguments(lib, weighted, loops, norm, directions):
    from rlap_amd import ops
    plan = ops.edge_list_plan(ROWS, [0, 2, 5], 4, weighted=weighted, add_self_loops=loops, fill_value=2.0, normalize=norm, directions=directions)
    (qname, q), (bname, b) = lib.exports()
    flags = (1 if weighted else 0) | (2 if loops else 0) | (4 if norm else 0) | DIRS[directions]
    assert qname == "rlap_snapshot_plan_bytes" and q == {"m": 5, "S": 2, "G": 1, "n": 4, "flags": flags}   # the layout's bound is the same
    assert bname == "rlap_edge_plan_build" and (b["m"], b["S"], b["G"], b["n"], b["flags"], b["fill"], b["plan_bytes"]) == (5, 2, 1, 4, flags, 2.0, BOUND)
    assert b["sc"] == ROWS.reshape(-1).tolist() and b["ptr"] == [0, 2, 5] and b["node_ptr"] is None
    assert isinstance(plan, ops.SnapshotPlan) and plan.nbytes == USED and (plan.layers, plan.num_nodes, plan.directions) == (2, 4, directions)
    assert ops.last_stats["host_syncs"] == 1 and ops.last_stats["blocks"] == 2 and ops.last_stats["arena_bytes"] == ARENA
    plan = ops.edge_list_plan(ROWS.float(), [0, 2, 5, 5], 4, [0, 2, 3, 4])                      # positional node_ptr, three graphs, one layer
    b = lib.exports()[-1][1]
    assert (b["G"], b["node_ptr"], b["flags"]) == (3, [0, 2, 3, 4], 2 | 4 | 768) and plan.layers == 1


def test_edge_plan_forms_the_rows_in_torch(lib):
    from rlap_amd import ops
    ei = torch.tensor([[2, 0, 2, 0, 3], [0, 1, 2, 1, 2]], dtype=torch.int32)
    w = torch.tensor([0.5, 0.5, 2.0, 0.25, 1.5], dtype=torch.float32)
    plan = ops.edge_plan(ei, w, directions="forward")
    b = lib.exports()[-1][1]
    assert lib.exports()[-1][0] == "rlap_edge_plan_build" and b["sc"] == ROWS.reshape(-1).tolist()
    assert (b["m"], b["S"], b["G"], b["n"], b["flags"], b["ptr"], b["node_ptr"]) == (5, 1, 1, 4, 1 | 2 | 4 | 256, [0, 5], None)   # max id + 1
    assert plan.layers == 1 and plan.num_nodes == 4
    ops.edge_plan(ei.long(), None, 9, add_self_loops=False, normalize=False, fill_value=3.0)
    b = lib.exports()[-1][1]
    assert (b["n"], b["flags"], b["fill"]) == (9, 768, 3.0) and b["sc"][2::3] == [1.0] * 5                  # unweighted: unit weights
    ops.edge_plan(torch.zeros((2, 0), dtype=torch.int64))
    b = lib.exports()[-1][1]
    assert (b["m"], b["n"], b["sc"], b["ptr"]) == (0, 0, None, [0, 0])


def test_host_checks_launch_nothing(lib):
    from rlap_amd import ops
    for kw, msg in [(dict(rows=ROWS[:, :2]), "sc: an"), (dict(rows=ROWS[0]), "sc: an"), (dict(num_nodes=-1), "num_nodes"),
                    (dict(num_nodes=2.5), "num_nodes"), (dict(ptr=[0, 2, 4]), "ptr"), (dict(ptr=[0, 3, 2, 5]), "ptr"), (dict(ptr=[0]), "ptr"),
                    (dict(node_ptr=[0, 1, 2, 4]), "node_ptr has 3 graphs"), (dict(node_ptr=[0, 5]), "node_ptr"),
                    (dict(fill_value=0.0), "fill_value"), (dict(fill_value=float("nan")), "fill_value"),
                    (dict(directions="backward"), "directions"), (dict(directions=None), "directions")]:
        a = dict(rows=ROWS, ptr=[0, 2, 5], num_nodes=4)
        a.update(kw)
        with pytest.raises(ValueError, match=msg):
            ops.edge_list_plan(a.pop("rows"), a.pop("ptr"), a.pop("num_nodes"), **a)
    ei = torch.tensor([[0, 1], [1, 0]])
    for args, kw, msg in [((ei.double(),), {}, "edge_index"), ((ei[0],), {}, "edge_index"), ((torch.zeros((3, 2), dtype=torch.int64),), {}, "edge_index"),
                          ((ei, torch.ones(3)), {}, "edge_weight"), ((ei, torch.ones(2, dtype=torch.int64)), {}, "edge_weight"),
                          ((ei, torch.ones(1, 2)), {}, "edge_weight"), ((ei,), dict(num_nodes=-2), "num_nodes"),
                          ((ei,), dict(fill_value=-1.0), "fill_value"), ((ei,), dict(directions="up"), "directions")]:
        with pytest.raises(ValueError, match=msg):
            ops.edge_plan(*args, **kw)
    assert lib.exports() == [] and ops.last_stats is None


@pytest.mark.parametrize("status,error,text", [(2, ValueError, "an id of the rows"), (3, ValueError, "a weight is not finite"),
                                               (9, RuntimeError, "status 9"), (10, RuntimeError, "status 10")])
def test_device_statuses_say_which(lib, status, error, text):
    from rlap_amd import ops
    lib.status = status
    with pytest.raises(error, match=text):
        ops.edge_list_plan(ROWS, [0, 5], 4, weighted=True)
    assert ops.last_stats is None and [c[0] for c in lib.exports()] == ["rlap_snapshot_plan_bytes", "rlap_edge_plan_build"]


def test_adapters_reach_the_edge_build(lib):
    from rlap_amd import adapters
    x = torch.ones(6, 3, dtype=torch.float64)
    ei = torch.tensor([[2, 0, 2, 0, 3], [0, 1, 2, 1, 2]])
    plan = adapters.graph_plan((x, ei, None), fill_value=2.0, directions="both")
    b = lib.exports()[-1][1]
    assert lib.exports()[-1][0] == "rlap_edge_plan_build" and (b["n"], b["flags"], b["fill"], b["m"]) == (6, 2 | 4 | 768, 2.0, 5)   # the loops cover x's ids
    plan = adapters.graph_plan(adapters.Graph(None, ei, torch.ones(5)))
    b = lib.exports()[-1][1]
    assert (b["n"], b["flags"]) == (4, 1 | 2 | 4 | 768)
    conv = adapters.SnapshotGCNConv(3, 2).double()
    out = conv(torch.ones(4, 3, dtype=torch.float64, requires_grad=True), plan)                       # a plan serves the conv by duck typing
    assert tuple(out.shape) == (1, 4, 2)
    out.sum().backward()
    assert [c[1]["flags"] for c in lib.exports()[-2:]] == [0, 16 | 64]
    assert "duck typing" in adapters.SnapshotGCNConv.__doc__


def test_export_in_header_exports_and_the_checked_call_path():
    from rlap_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "rlap_edge_plan_build" in _lib.EXPORTS

    def args(name):
        return re.sub(r"\s+", " ", re.search(r"\bint %s\(([^)]*)\);" % name, hdr).group(1))
    assert args("rlap_edge_plan_build") == args("rlap_snapshot_plan_build")      # one argument list, rlap_plan_desc and rlap_plan_info
    api = open(os.path.join(INC, "rlap_api.hip")).read()
    body = api[api.index("int rlap_edge_plan_build("):api.index("int rlap_snapshot_plan_propagate(")]
    assert "snapshot_check(h, &g, 1)" in body and "return snapshot_call(h," in body and "edge_plan_build_run(" in body
    assert "*h_desc = rlap_plan_desc{};" in body and "hipMalloc" not in body
    src = open(os.path.join(INC, "rlap_edgeplan.hip")).read()
    assert "hipMalloc" not in src and "hipStreamSynchronize" in src and src.count("hipStreamSynchronize(") == 1   # scratch from the arena; one synchronisation
    assert not re.search(r"atomic\w*\([^;]*(double|float)", src)
    mk = open(os.path.join(INC, "Makefile")).read()
    assert "rlap_edgeplan.o" in mk and "rlap_edgeplan.h" in mk and "-ffp-contract=off" in mk and "fast-math" not in mk
