"""Markov diffusion without a GPU (ops.snapshot_markov, ops.markov_diffusion):

  a. the host mirror (tests/csrc/markov_mirror.cc: rlap_amd/csrc/rlap_markov.h compiled with g++, the rule run sparsely in the
     device's order) against the dense restatement in numpy float64 in the published loop's order (tests/markov_mirror.py::dense):
     the keep pattern exactly, every kept value within relative 2 (D + 2) (n + 4) 2^-53.  A >= 0, so every entry is a sum of
     non-negative products; the bound counts the roundings of D + 2 sweeps with sums of at most n + 4 terms on either side.  Before
     patterns are compared every case ASSERTS that no dense entry lies within relative 1e-9 of eps (random symmetric weights and an
     eps that is no round decimal keep them apart);
  b. closed forms, ids without edges, duplicates, symmetry, normalize_out, adapters.compute_markov_diffusion against the same dense;
  c. tests/csrc/markov_main.cc as a stand-alone program under -fsanitize=address,undefined (the tile table is the PPR diffusion's,
     untouched: tests/test_ppr_tiles_cpu.py);
  d. the entry points on the stub library: every ValueError, the capacity guess and the retry, node_ptr segmentation of both
     diffusions, rLapDepths.diffuse(kind=...), MarkovDiffusion's cache;
  e. rlap_markov_info against _lib.MarkovInfo, and the export list.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import markov_mirror as mm
from rlap_amd import _lib, adapters, ops
from util import StubLib, ba_graph, f64_at, i64_at, path, star, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1.2345e-3   # no round decimal


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return mm.build(tmp_path_factory.mktemp("markov"))


def bound(n, D):
    return 2 * (D + 2) * (n + 4) * 2.0 ** -53


def check_against_dense(lib, sc, alpha=0.2, order=16, eps=EPS, weighted=True, self_loop=True, zero_ok=False):
    """Mirror against dense: (raw, norm, nodes, M).  Asserts the gap first, then pattern, values, order and exact symmetry."""
    nodes, M = mm.dense(sc, alpha, order, weighted, self_loop)
    n = len(nodes)
    assert not np.any(np.abs(M - eps) <= 1e-9 * eps), "a dense entry lies within 1e-9 of eps: the keep decision is not determined"
    raw, norm = mm.run(lib, sc, alpha, order, eps, weighted, self_loop, zero_ok)
    got, keep = mm.to_dense(raw, nodes)
    assert np.array_equal(keep, M >= eps), "the keep pattern differs"
    if keep.any():
        rel = float((np.abs(got - M)[keep] / M[keep]).max())
        print(f"n={n} D={order} loop={self_loop}: max rel diff {rel:.3g}, bound {bound(n, order):.3g}")
        assert rel <= bound(n, order)
    key = raw[:, 0].astype(np.int64) * (int(nodes.max()) + 1 if n else 1) + raw[:, 1].astype(np.int64)
    assert np.all(key[1:] > key[:-1]), "rows are not in ascending (i, j) order"
    assert np.array_equal(got, got.T), "not exactly symmetric"
    gn, _ = mm.to_dense(norm, nodes)
    assert np.array_equal(gn, gn.T)
    want = mm.threshold(M, eps, True)
    assert np.allclose(gn, want, rtol=4 * bound(n, order) + 2.0 ** -48, atol=0.0)
    return raw, norm, nodes, M


# ------------------------------------------------------------------------------------------------ a. mirror against dense
@pytest.mark.parametrize("n", [2, 7, 65, 128, 300, 1000])
@pytest.mark.parametrize("D", [1, 2, 16])
@pytest.mark.parametrize("loop", [False, True])
def test_mirror_against_dense_random_weights(lib, n, D, loop):
    ei = np.array([[0, 1], [1, 0]]) if n == 2 else np.asarray(ba_graph(n, 3, n))
    sc = mm.column_layout(ei, mm.symmetric_weights(ei, 5 + n))
    check_against_dense(lib, sc, order=D, self_loop=loop)


@pytest.mark.parametrize("n,D", [(60, 3), (200, 16), (129, 2)])
def test_mirror_against_dense_unit_weights(lib, n, D):
    """weighted=False ignores the rows' weights; with unit entries a round eps can fall on an entry exactly, so eps is irrational-ish
    and the gap is asserted like everywhere."""
    ei = np.asarray(ba_graph(n, 2, 3))
    sc = mm.column_layout(ei, mm.symmetric_weights(ei, 1))
    a = check_against_dense(lib, sc, order=D, weighted=False, eps=0.7391e-3)[0]
    sc[:, 2] = 1.0
    b = check_against_dense(lib, sc, order=D, weighted=True, eps=0.7391e-3)[0]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("D", [1, 2, 3, 16])
@pytest.mark.parametrize("alpha", [0.0, 0.2, 1.0])
def test_orders_and_alphas(lib, D, alpha):
    """Both parities of the final copy; alpha = 0 (beta = 1: the plain power sum) and alpha = 1 (beta = 0: (alpha + 1/D) Â)."""
    assert lib.markov_final_copy(D) == (0 if D & 1 else 1)
    ei = np.asarray(ba_graph(90, 3, 8))
    sc = mm.column_layout(ei, mm.symmetric_weights(ei, 2))
    raw, _, nodes, M = check_against_dense(lib, sc, alpha=alpha, order=D)
    if alpha == 1.0:
        _, ah = mm.dense(sc, 1.0, 1)                      # order 1 at alpha 1: M = 2 Â
        got, keep = mm.to_dense(raw, nodes)
        assert np.allclose(got[keep], ((1.0 + 1.0 / D) * ah / 2.0)[keep], rtol=1e-14, atol=0)


def test_a_subset_of_the_tiles(lib):
    ei = np.asarray(ba_graph(200, 3, 4))
    sc = mm.column_layout(ei, mm.symmetric_weights(ei, 9))
    raw, _ = mm.run(lib, sc, eps=EPS)
    part, _ = mm.run(lib, sc, eps=EPS, tiles=[0, 2])
    lo = np.minimum(raw[:, 0], raw[:, 1])                 # (columns are in id order here: tile t is ids 64 t .. 64 t + 63)
    assert 0 < part.shape[0] < raw.shape[0] and np.array_equal(part, raw[(lo < 64) | ((lo >= 128) & (lo < 192))])


# ------------------------------------------------------------------------------------------------ b. closed forms and edge cases
def geo(beta, D):
    return sum(beta ** k for k in range(D + 1))


@pytest.mark.parametrize("D", [1, 2, 3, 16])
def test_one_loop_row(lib, D):
    raw, norm = mm.run(lib, [[7, 7, 4.0]], alpha=0.2, order=D, self_loop=False)
    assert raw[:, :2].tolist() == [[7, 7]] and raw[0, 2] == pytest.approx(0.2 + geo(0.8, D) / D, rel=1e-14)
    assert norm[0, 2] == pytest.approx(1.0, rel=1e-15)


def test_two_nodes(lib):
    D, a, b = 3, 0.25, 0.75
    raw, _ = mm.run(lib, [[1, 0, 3.0], [0, 1, 3.0]], alpha=a, order=D, eps=1e-6, self_loop=False)
    off, dia = a + (1 + b * b) / D, (b + b ** 3) / D
    assert raw[:, :2].tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    assert raw[:, 2] == pytest.approx([dia, off, off, dia], rel=1e-14) and raw[1, 2] == raw[2, 2]


def test_star_closed_form(lib):
    """A star of k leaves without the loop: Â^2 restricted to the leaves is (1/k) 1 1^T, and Â^(2p+1) = Â -- so for D = 2:
    hub-leaf = (alpha + (1 + beta^2) / 2) / sqrt(k), hub-hub = beta / 2, leaf-leaf = beta / (2 k)."""
    k, a = 9, 0.2
    b = 1 - a
    sc = mm.column_layout(star(k + 1))
    raw, _ = mm.run(lib, sc, alpha=a, order=2, eps=1e-6, self_loop=False)
    nodes = np.arange(k + 1)
    got, keep = mm.to_dense(raw, nodes)
    assert keep.all()
    assert got[0, 0] == pytest.approx(b / 2, rel=1e-14)
    assert got[0, 1:] == pytest.approx(np.full(k, (a + (1 + b * b) / 2) / 3.0), rel=1e-14)
    assert got[1:, 1:] == pytest.approx(np.full((k, k), b / (2 * k)), rel=1e-14)


@pytest.mark.parametrize("D", [2, 5])
def test_an_id_without_edges(lib, D):
    sc = np.array([[1, 0, 1.5], [0, 1, 1.5], [5, 5, 0.0]])
    with pytest.raises(mm.Refused):
        mm.run(lib, sc, order=D)                          # a zero weight needs the flag
    raw, _ = mm.run(lib, sc, order=D, self_loop=False, zero_ok=True)
    assert 5 not in raw[:, :2] and raw.shape[0] == 4      # its Â row is zero: no row at all
    raw, norm = mm.run(lib, sc, order=D, self_loop=True, zero_ok=True)
    row = raw[raw[:, 0] == 5]
    assert row[:, :2].tolist() == [[5, 5]] and row[0, 2] == pytest.approx(0.2 + geo(0.8, D) / D, rel=1e-14)
    check_against_dense(lib, sc, order=D, self_loop=True, zero_ok=True, eps=1e-4)


def test_duplicates_are_summed_in_input_order(lib):
    """The degree is the row-order sum of the rows: (1e16 + 1) + 1 differs from 1e16 + (1 + 1) in float64, and the mirror (as the
    device) takes the first.  Against one summed row the values agree to rounding."""
    big = 1e16
    sc = np.array([[1, 0, big], [1, 0, 1.0], [1, 0, 1.0], [0, 1, big], [0, 1, 1.0], [0, 1, 1.0]])
    raw, _ = mm.run(lib, sc, order=2, self_loop=False, eps=1e-6)
    one = np.array([[1, 0, big + 2.0], [0, 1, big + 2.0]])
    ref, _ = mm.run(lib, one, order=2, self_loop=False, eps=1e-6)
    assert np.array_equal(raw[:, :2], ref[:, :2]) and np.allclose(raw[:, 2], ref[:, 2], rtol=1e-15, atol=0)
    small = np.array([[1, 0, 0.5], [1, 0, 0.25], [0, 1, 0.25], [0, 1, 0.5], [2, 2, 1.0]])
    check_against_dense(lib, small, order=3, eps=1e-4)


def test_the_adapter_restatement_is_the_dense_loop():
    ei = np.asarray(ba_graph(80, 3, 6))
    w = mm.symmetric_weights(ei, 4)
    for loop in (False, True):
        for norm in (False, True):
            idx, val = adapters.compute_markov_diffusion(torch.from_numpy(ei), torch.from_numpy(w), 80, alpha=0.2, degree=5, sp_eps=EPS,
                                                         add_self_loop=loop, normalize_out=norm)
            _, M = mm.dense(mm.column_layout(ei, w), 0.2, 5, True, loop)
            want = mm.threshold(M, EPS, norm)
            got = np.zeros((80, 80))
            got[idx[0].numpy(), idx[1].numpy()] = val.numpy()
            assert np.array_equal(got != 0, want != 0) and np.allclose(got, want, rtol=1e-12, atol=0)
            key = idx[0] * 80 + idx[1]
            assert bool((key[1:] > key[:-1]).all())


# ------------------------------------------------------------------------------------------------ c. stand-alone programs
SAN = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
       "-fno-omit-frame-pointer", "-ffp-contract=off", "-I", os.path.join(ROOT, "rlap_amd", "csrc")]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def test_the_mirror_under_asan_ubsan(tmp_path):
    exe = tmp_path / "markov_main"
    subprocess.check_call(SAN + ["-o", str(exe), mm.MAIN])
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=SAN_ENV, timeout=300)
    assert r.returncode == 0 and "\n0 failures" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ d. entry points on the stub
HEAD = "h sc m ptr S node_ptr G n "
SIGS = {"rlap_snapshot_markov": HEAD + "alpha order eps flags out cap out_ptr info",
        "rlap_snapshot_ppr": HEAD + "alpha eps tol flags out cap out_ptr info"}
ARENA = 4321


class Stub(StubLib):
    def __init__(self):
        super().__init__(SIGS)
        self.statuses, self.rows = [], 3

    def export(self, name, a):
        m, S, G = a["m"], a["S"], a["G"]
        rec = {k: a[k] for k in ("m", "S", "G", "n", "alpha", "eps", "flags", "cap")}
        rec["order"] = a.get("order")
        rec["sc"] = None if a["sc"] is None else f64_at(a["sc"], 3 * min(m, 64))
        rec["ptr"] = i64_at(a["ptr"], S + 1)
        rec["node_ptr"] = None if a["node_ptr"] is None else i64_at(a["node_ptr"], G + 1)
        rec["out_null"] = a["out"] is None
        self.calls.append((name, rec))
        status = self.statuses.pop(0) if self.statuses else self.status
        info = a["info"]._obj
        info.rows_needed = self.rows
        if status:
            return status
        info.host_syncs, info.arena_bytes = 3, ARENA
        if name == "rlap_snapshot_markov":
            info.order, info.small_tiles, info.groups, info.launches = a["order"], S, 1, 5
        out = ctypes.cast(a["out"] or 0, ctypes.POINTER(ctypes.c_double))
        for r in range(self.rows):
            out[3 * r], out[3 * r + 1], out[3 * r + 2] = float(r), float(r), 0.25
        optr = ctypes.cast(a["out_ptr"], ctypes.POINTER(ctypes.c_int64))
        for s in range(S + 1):
            optr[s] = 0 if s == 0 else self.rows
        return 0


@pytest.fixture
def stub(monkeypatch):
    return stub_ops(monkeypatch, Stub())


SC = torch.tensor([[1, 0, 0.5], [0, 1, 0.5], [3, 2, 2.0], [2, 3, 2.0], [2, 2, 1.5]], dtype=torch.float64)
PTR, M, N = [0, 2, 5], 5, 4


@pytest.mark.parametrize("weighted,loop,norm", [(True, True, False), (False, False, True), (True, False, True), (False, True, False)])
def test_snapshot_markov_arguments(stub, weighted, loop, norm):
    out, mptr = ops.snapshot_markov(SC, PTR, N, alpha=0.3, order=7, eps=1e-3, weighted=weighted, add_self_loop=loop, normalize_out=norm)
    (name, rec), = stub.exports()
    assert name == "rlap_snapshot_markov" and (rec["m"], rec["S"], rec["G"], rec["n"], rec["node_ptr"]) == (M, 2, 1, N, None)
    assert rec["sc"] == SC.reshape(-1).tolist() and rec["ptr"] == PTR
    assert (rec["alpha"], rec["order"], rec["eps"]) == (0.3, 7, 1e-3)
    assert rec["flags"] == (1 if weighted else 0) | (2 if loop else 0) | (4 if norm else 0)
    assert rec["cap"] == 2 * min(N, M) ** 2 and not rec["out_null"]
    assert out.tolist() == [[0.0, 0.0, 0.25], [1.0, 1.0, 0.25], [2.0, 2.0, 0.25]] and mptr.tolist() == [0, 3, 3]
    assert ops.last_stats == {"order": 7, "small_tiles": 2, "large_tiles": 0, "groups": 1, "launches": 5, "rows_needed": 3,
                              "arena_bytes": ARENA, "host_syncs": 3, "output_retries": 0, "first_cap": 32}


def test_snapshot_markov_defaults_and_capacity(stub):
    ops.snapshot_markov(SC, PTR, N, node_ptr=[0, 2, 4])
    rec = stub.exports()[0][1]
    assert (rec["alpha"], rec["order"], rec["eps"], rec["flags"], rec["G"], rec["node_ptr"], rec["cap"]) == (0.2, 16, 1e-4, 1 | 2, 2, [0, 2, 4], 32)
    stub.rows = 0
    out, _ = ops.snapshot_markov(torch.zeros((0, 3), dtype=torch.float64), [0, 0], 9)
    rec = stub.exports()[1][1]
    assert rec["cap"] == 0 and rec["out_null"] and rec["sc"] is None and tuple(out.shape) == (0, 3)
    big = torch.ones((1 << 19, 3), dtype=torch.float64)
    ops.snapshot_markov(big, [0, 1 << 19], 1 << 12)
    assert stub.exports()[2][1]["cap"] == 16 * (1 << 19) + 64
    ops.snapshot_markov(big[:4096], [0, 4096], 1 << 12)
    assert stub.exports()[3][1]["cap"] == 1 << 22


def test_snapshot_markov_retries_once(stub):
    stub.rows, stub.statuses = 40, [_lib.E_OUT_CAPACITY]
    out, _ = ops.snapshot_markov(SC, PTR, N)
    assert [c[1]["cap"] for c in stub.exports()] == [32, 40] and tuple(out.shape) == (40, 3)
    assert ops.last_stats["output_retries"] == 1 and ops.last_stats["first_cap"] == 32 and ops.last_stats["rows_needed"] == 40
    before = dict(ops.last_stats)
    stub.statuses = [_lib.E_OUT_CAPACITY, _lib.E_OUT_CAPACITY, 0]
    with pytest.raises(RuntimeError, match=r"rlap: status 13"):
        ops.snapshot_markov(SC, PTR, N)
    assert len(stub.exports()) == 4 and ops.last_stats == before


@pytest.mark.parametrize("kw", [
    {"alpha": -0.1}, {"alpha": 1.5}, {"alpha": float("nan")}, {"alpha": True}, {"alpha": "0.2"},
    {"order": 0}, {"order": -3}, {"order": 1025}, {"order": 2.5}, {"order": True},
    {"eps": 0.0}, {"eps": -1e-4}, {"eps": float("nan")}, {"eps": float("inf")},
])
def test_bad_parameters_launch_nothing(stub, kw):
    with pytest.raises(ValueError):
        ops.snapshot_markov(SC, PTR, N, **kw)
    with pytest.raises(ValueError):
        ops.markov_diffusion(SC[:2, :2].long().t(), None, 2, **kw)
    assert stub.exports() == []


def test_the_limits_are_allowed(stub):
    for kw in ({"alpha": 0}, {"alpha": 1}, {"alpha": 1.0}, {"order": 1}, {"order": 1024}):
        ops.snapshot_markov(SC, PTR, N, **kw)
    assert len(stub.exports()) == 5 and ops.MARKOV_MAX_ORDER == 1024


@pytest.mark.parametrize("args,kw", [
    ((SC, [0, 3], N), {}), ((SC, [1, 5], N), {}), ((SC, [0, 4, 2, 5], N), {}), ((SC, PTR, -1), {}), ((SC[:, :2], PTR, N), {}),
    ((SC, PTR, N), {"node_ptr": [0, 1, 2, 4]}), ((SC, PTR, N), {"node_ptr": [0, 3]}),
    ((torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64), [0, 2], 2), {}),
    ((torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0]], dtype=torch.float64), [0, 2], 2), {}),
    ((torch.tensor([[1.0, 0.0, float("inf")], [0.0, 1.0, float("inf")]], dtype=torch.float64), [0, 2], 2), {}),
])
def test_bad_tables_and_weights(stub, args, kw):
    with pytest.raises(ValueError):
        ops.snapshot_markov(*args, **kw)
    assert stub.exports() == []


@pytest.mark.parametrize("status", [1, 2, 3, 12, 5])
def test_statuses_become_exceptions(stub, status):
    stub.status = status
    value_error = status in (1, 2, 3, 12)
    with pytest.raises(ValueError if value_error else RuntimeError) as e:
        ops.snapshot_markov(SC, PTR, N)
    assert str(e.value).startswith(f"rlap: status {status}") and (status != 3 or str(e.value).endswith("(or a weight is <= 0)"))


# two graphs over ids 0..2 and 3..6 (id 6 without edges), rows in no particular order, one duplicate
EI = torch.tensor([[4, 0, 1, 3, 1, 2, 5, 4, 0, 1], [3, 1, 0, 4, 2, 1, 4, 5, 1, 0]])
EW = torch.tensor([1.0, 2.0, 2.0, 1.0, 3.0, 3.0, 0.5, 0.5, 0.25, 0.25])
ROWS = [1.0, 0.0, 2.25, 0.0, 1.0, 2.25, 2.0, 1.0, 3.0, 1.0, 2.0, 3.0,      # graph 0, grouped by column
        4.0, 3.0, 1.0, 3.0, 4.0, 1.0, 5.0, 4.0, 0.5, 4.0, 5.0, 0.5, 6.0, 6.0, 0.0]


@pytest.mark.parametrize("which", ["markov", "ppr"])
def test_diffusions_with_and_without_node_ptr(stub, which):
    fn = ops.markov_diffusion if which == "markov" else ops.ppr_diffusion
    zero_rows, weighted = 8, 1
    idx, w = fn(EI, EW, 7)
    name, rec = stub.exports()[0]
    assert name == f"rlap_snapshot_{which}" and (rec["m"], rec["S"], rec["G"], rec["n"], rec["node_ptr"], rec["ptr"]) == (9, 1, 1, 7, None, [0, 9])
    assert rec["sc"] == ROWS and rec["flags"] == (weighted | zero_rows | 2 if which == "markov" else weighted | zero_rows | 4)
    assert rec["cap"] == 49
    assert idx.tolist() == [[0, 1, 2], [0, 1, 2]] and w.tolist() == [0.25] * 3
    fn(EI, EW, 7, node_ptr=[0, 3, 7])
    rec = stub.exports()[1][1]
    assert (rec["m"], rec["S"], rec["G"], rec["n"], rec["node_ptr"], rec["ptr"]) == (9, 2, 2, 7, [0, 3, 7], [0, 4, 9]) and rec["sc"] == ROWS
    assert rec["cap"] == 2 * 49                                             # S min(n, m)^2, an upper bound still
    fn(EI, EW, 7, node_ptr=torch.tensor([0, 3, 6, 7]))                      # a graph of one id without edges
    assert stub.exports()[2][1]["ptr"] == [0, 4, 8, 9]
    fn(EI, EW, 7, node_ptr=[0, 0, 3, 7, 7])                                 # empty graphs
    assert stub.exports()[3][1]["ptr"] == [0, 0, 4, 9, 9]
    with pytest.raises(ValueError, match="joins two graphs"):
        fn(EI, EW, 7, node_ptr=[0, 2, 7])                                   # the row 1 - 2 crosses
    with pytest.raises(ValueError, match="node_ptr"):
        fn(EI, EW, 7, node_ptr=[0, 3, 6])                                   # does not end at num_nodes
    with pytest.raises(ValueError, match="not symmetric"):
        fn(EI[:, :-1], EW[:-1], 7, node_ptr=[0, 3, 7])
    assert len(stub.exports()) == 4


def test_markov_diffusion_arguments(stub):
    ops.markov_diffusion(EI, None, 7, alpha=0.5, order=3, eps=1e-2, add_self_loop=False, normalize_out=True)
    rec = stub.exports()[0][1]
    assert (rec["alpha"], rec["order"], rec["eps"], rec["flags"]) == (0.5, 3, 1e-2, 1 | 8 | 4)
    assert rec["sc"][2] == 2.0                                               # unit weights: the duplicate 1 -> 0 counts twice


class FakeDepths(adapters.rLapDepths):
    def _snapshots(self, g):
        return torch.zeros(N, 2), SC, torch.tensor(PTR), N


def test_depths_diffuse_kind(stub, monkeypatch):
    d = FakeDepths(fracs=(0.1, 0.2))
    gs = d.diffuse(None)
    assert stub.exports()[0][0] == "rlap_snapshot_ppr" and len(gs) == 2      # the default is unchanged
    gs = d.diffuse(None, alpha=0.3, eps=1e-3, kind="markov", order=5)
    name, rec = stub.exports()[1]
    assert name == "rlap_snapshot_markov" and (rec["alpha"], rec["order"], rec["eps"], rec["flags"]) == (0.3, 5, 1e-3, 1 | 2)
    assert len(gs) == 2 and gs[0].edge_index.tolist() == [[0, 1, 2], [0, 1, 2]] and gs[1].edge_index.shape == (2, 0)
    with pytest.raises(ValueError, match="kind"):
        d.diffuse(None, kind="heat")
    seen = []
    monkeypatch.setattr(ops, "edge_list_plan", lambda out, pptr, n, **kw: seen.append((tuple(out.shape), pptr.tolist(), n, kw)) or "plan")
    assert d.diffuse_plan(None, kind="markov", order=2) == "plan" and stub.exports()[2][1]["order"] == 2
    assert d.diffuse_plan(None) == "plan" and stub.exports()[3][0] == "rlap_snapshot_ppr"
    assert seen[0][:3] == ((3, 3), [0, 3, 3], N) and seen[0][3]["weighted"] is True


def test_markov_diffusion_adapter_caches_like_pygcl(stub):
    aug = adapters.MarkovDiffusion()
    assert (aug.alpha, aug.order, aug.sp_eps, aug.use_cache, aug.add_self_loop) == (0.05, 16, 1e-4, True, True)
    x = torch.zeros(7, 2)
    g1 = aug(x, EI, EW)
    g2 = aug(x, EI, EW)
    assert g1 is g2 and len(stub.exports()) == 1
    rec = stub.exports()[0][1]
    assert (rec["alpha"], rec["order"], rec["eps"], rec["n"], rec["S"]) == (0.05, 16, 1e-4, 7, 1)
    res = g1.unfold() if hasattr(g1, "unfold") else g1
    assert res[0] is x and res[1].tolist() == [[0, 1, 2], [0, 1, 2]]
    fresh = adapters.MarkovDiffusion(alpha=0.2, order=4, sp_eps=1e-3, use_cache=False, add_self_loop=False)
    fresh(x, EI, EW, node_ptr=adapters.node_ptr_of(torch.tensor([0, 0, 0, 1, 1, 1, 1])))
    fresh(x, EI, EW)
    assert len(stub.exports()) == 3
    rec = stub.exports()[1][1]
    assert (rec["S"], rec["G"], rec["node_ptr"], rec["order"], rec["flags"]) == (2, 2, [0, 3, 7], 4, 1 | 8)


# ------------------------------------------------------------------------------------------------ e. layout and exports
def test_layout_matches_the_header(tmp_path):
    """_lib.MarkovInfo and rlap_markov_info describe the same bytes (the method of tests/test_cabi_symbols.py)."""
    import shutil
    gcc = shutil.which("gcc")
    assert gcc, "gcc is needed to check the C layout"
    c_name, cls = "rlap_markov_info", _lib.MarkovInfo
    fields = [f for f, _ in cls._fields_]
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    end = hdr.index("} %s;" % c_name)
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [name for decl in re.findall(r"\b(?:int32_t|int64_t|float|double)\s+([a-z_0-9, ]+);", body) for name in decl.split(", ")]
    assert declared == fields
    src = tmp_path / "layout.c"
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rlap_hip.h"', "int main(void) {",
             f'    printf("sizeof %zu\\n", sizeof({c_name}));']
    lines += [f'    printf("{f} %zu\\n", offsetof({c_name}, {f}));' for f in fields]
    lines += ["    return 0;", "}"]
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got.pop("sizeof")) == ctypes.sizeof(cls)
    assert {f: int(v) for f, v in got.items()} == {f: getattr(cls, f).offset for f in fields}


def test_export_flags_and_limits(lib):
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "rlap_snapshot_markov" in _lib.EXPORTS and re.search(r"\bint rlap_snapshot_markov\(", hdr)
    flags = dict(re.findall(r"RLAP_MARKOV_([A-Z_]+) = (\d+)", hdr))
    assert {k: int(v) for k, v in flags.items()} == {"WEIGHTED": _lib.MARKOV_WEIGHTED, "SELF_LOOP": _lib.MARKOV_SELF_LOOP,
                                                     "NORMALIZE": _lib.MARKOV_NORMALIZE, "ZERO_ROWS": _lib.MARKOV_ZERO_ROWS}
    assert lib.markov_max_order() == _lib.MARKOV_MAX_ORDER == ops.MARKOV_MAX_ORDER
    for alpha, order, eps, ok in [(0.0, 1, 1e-4, 1), (1.0, 1024, 1e-300, 1), (-1e-9, 1, 1e-4, 0), (1.0000001, 1, 1e-4, 0), (0.2, 0, 1e-4, 0),
                                  (0.2, 1025, 1e-4, 0), (0.2, 16, 0.0, 0), (0.2, 16, float("inf"), 0), (float("nan"), 16, 1e-4, 0)]:
        assert lib.markov_valid(alpha, order, eps) == ok
