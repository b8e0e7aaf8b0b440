"""The Python -> C mapping of every elimination entry point, without a GPU: the device is the CPU and the library a stub that
records each call with its arguments (host tables read through their addresses) and writes a result of its own."""
import ctypes

import pytest
import torch

from rlap_amd import ops
from util import StubLib, i64_at as i64, stub_ops

# positional arguments of the six exports (include/rlap_hip.h)
SIGS = {
    "rlap_approx_chol": "h row col w E n t o_v o_n perm seed out cap rows st",
    "rlap_approx_chol_from_edges": "h row col w E n t frac sym o_v o_n perm seed out cap rows nn st",
    "rlap_approx_chol_batched": "h row col w E G node_ptr num_remove o_v o_n perm seed out cap ptr st",
    "rlap_approx_chol_views": "h row col w E G node_ptr K num_remove o_v o_n perm seed out cap ptr st",
    "rlap_approx_chol_depths": "h row col w E n D num_remove o_v o_n perm seed out cap ptr st",
    "rlap_approx_chol_views_depths": "h row col w E G node_ptr K D num_remove o_v o_n perm seed out cap ptr st",
}
NN = 37   # num_nodes the stub "finds" for rlap_approx_chol_from_edges with n < 0


class ElimStub(StubLib):
    def export(self, name, a):
        rec = {k: a[k] for k in ("E", "o_v", "o_n", "seed", "cap")}
        E = a["E"]
        rec["rows"] = (i64(a["row"], E), i64(a["col"], E))
        rec["weighted"] = a["w"] is not None
        G, K, D = a.get("G", 1), a.get("K", 1), a.get("D", 0)
        if "node_ptr" in a:
            rec["node_ptr"] = i64(a["node_ptr"], G + 1)
            n = rec["node_ptr"][-1]
        else:
            n = a["n"]
        rec.update(n=n, G=G, K=K, D=D)
        if "num_remove" in a:
            rec["num_remove"] = i64(a["num_remove"], max(D, 1) * K * G)
        else:
            rec["num_remove"] = [a["t"]]
        if name == "rlap_approx_chol_from_edges":
            rec.update(frac=a["frac"], sym=a["sym"])
        rec["perm"] = None if a["perm"] is None else i64(a["perm"], K * (NN if n < 0 else n))
        self.calls.append((name, rec))
        if self.status:
            return self.status
        # the stub's result: segment i holds one row (as far as the capacity goes), row r = [r, r + 1, 0.5]
        segs = max(D, 1) * K * G
        ptr = [min(i, a["cap"]) for i in range(segs + 1)]
        rows = ptr[-1]
        out = ctypes.cast(a["out"], ctypes.POINTER(ctypes.c_double))
        for r in range(rows):
            out[3 * r], out[3 * r + 1], out[3 * r + 2] = float(r), float(r + 1), 0.5
        if "ptr" in a:
            p = ctypes.cast(a["ptr"], ctypes.POINTER(ctypes.c_int64))
            for i, v in enumerate(ptr):
                p[i] = v
        else:
            a["rows"]._obj.value = rows
        if "nn" in a:
            a["nn"]._obj.value = NN if a["n"] < 0 else a["n"]
        a["st"]._obj.out_rows = rows
        a["st"]._obj.n_eliminated = 1000 + rows
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, ElimStub(SIGS))


def path(n):
    a = torch.arange(n - 1)
    return torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])])


def exports(stub):
    return stub.exports()


def queries(stub):
    return [c[1]["args"] for c in stub.calls if c[0] == "rlap_workspace_query"]


def rng_modes(stub):
    return [c[1]["mode"] for c in stub.calls if c[0] == "rlap_set_rng_mode"]


def drawn_seed(s):
    torch.manual_seed(s)
    return int(torch.randint(0, 2**62, (1,)).item())


def untouched_rng(s):
    """True when nothing drew from torch's RNG since torch.manual_seed(s)."""
    v = int(torch.randint(0, 2**62, (1,)).item())
    return v == drawn_seed(s)


def check_result(res, rec, segs):
    rows = min(segs, rec["cap"])
    assert res.dtype == torch.float64 and tuple(res.shape) == (rows, 3)
    assert res[:, 0].tolist() == [float(r) for r in range(rows)] and res[:, 2].tolist() == [0.5] * rows
    assert ops.last_stats["out_rows"] == rows and ops.last_stats["n_eliminated"] == 1000 + rows


def the_call(stub):
    calls = exports(stub)
    assert len(calls) == 1, calls
    return calls[0]


def test_approximate_cholesky(lib):
    ei = path(10)
    E = ei.shape[1]
    w = torch.rand(E, dtype=torch.float64)
    res = ops.approximate_cholesky(ei, w, 10, 4, "degree", "asc", seed=5)
    name, rec = the_call(lib)
    assert name == "rlap_approx_chol"
    assert (rec["E"], rec["n"], rec["G"], rec["K"], rec["D"], rec["num_remove"]) == (E, 10, 1, 1, 0, [4])
    assert (rec["o_v"], rec["o_n"], rec["seed"], rec["perm"], rec["cap"], rec["weighted"]) == (1, 0, 0, None, E, True)
    assert rec["rows"] == (ei[0].tolist(), ei[1].tolist())
    assert queries(lib) == [(E, 10, 1, 0)] and rng_modes(lib) == [0]
    check_result(res, rec, 1)
    assert res.device.type == "cpu"


@pytest.mark.parametrize("o_v,o_n,mode,draws", [("degree", "asc", "exact", False), ("degree", "desc", "exact", False),
                                                ("degree", "random", "exact", True), ("random", "asc", "exact", True),
                                                ("coarsen", "asc", "exact", True), ("degree", "asc", "frontier", True)])
def test_when_the_seed_is_drawn(lib, o_v, o_n, mode, draws):
    ei = path(12)
    torch.manual_seed(31)
    ops.approximate_cholesky(ei, None, 12, 5, o_v, o_n, mode=mode)
    rec = the_call(lib)[1]
    assert rec["seed"] == (drawn_seed(31) if draws else 0)
    assert rng_modes(lib) == [1 if mode == "frontier" else 0]
    torch.manual_seed(31)
    ops.approximate_cholesky(ei, None, 12, 5, o_v, o_n, mode=mode, seed=2**64 + 9)
    assert exports(lib)[1][1]["seed"] == (9 if draws else 0)
    assert untouched_rng(31)


def test_approximate_cholesky_perm_and_return_device(lib):
    ei = path(10)
    perm = torch.randperm(10)
    res = ops.approximate_cholesky(ei, None, 10, 3, "random", "random", perm=perm.int(), seed=8, return_device="meta")
    rec = the_call(lib)[1]
    assert (rec["o_v"], rec["o_n"], rec["seed"], rec["perm"]) == (0, 2, 8, perm.tolist())
    assert res.device.type == "meta" and tuple(res.shape) == (1, 3)
    res = ops.approximate_cholesky(ei, None, 10, 3, "degree", "asc", perm=perm)   # (perm is read for o_v="random" only)
    assert exports(lib)[1][1]["perm"] is None
    with pytest.raises(AssertionError):
        ops.approximate_cholesky(ei, None, 10, 3, "random", "asc", perm=perm[:9])
    with pytest.raises(AssertionError):
        ops.approximate_cholesky(ei, None, 10, 3, "bogus", "asc")
    with pytest.raises(AssertionError):
        ops.approximate_cholesky(ei, None, 10, 3, "degree", "bogus")
    assert len(exports(lib)) == 2


def test_no_edges(lib):
    ei = torch.zeros((2, 0), dtype=torch.int64)
    res = ops.approximate_cholesky(ei, None, 4, 2, "degree", "asc")
    rec = the_call(lib)[1]
    assert (rec["E"], rec["cap"]) == (0, 1) and queries(lib) == [(0, 4, 1, 0)]
    check_result(res, rec, 1)


def test_a_failed_call_leaves_last_stats(lib):
    ops.approximate_cholesky(path(10), None, 10, 3, "degree", "asc")
    before = dict(ops.last_stats)
    lib.status = 3
    with pytest.raises(ValueError):
        ops.approximate_cholesky(path(10), None, 10, 4, "degree", "asc")
    lib.status = 5
    with pytest.raises(RuntimeError):
        ops.approximate_cholesky_views(path(10), None, 10, [1, 2], "degree", "asc")
    assert ops.last_stats == before and len(exports(lib)) == 3


def test_from_edges_found_num_nodes(lib):
    ei = path(20)[:, :19]   # one direction of every edge
    E = ei.shape[1]
    torch.manual_seed(4)
    res, nn = ops.approximate_cholesky_from_edges(ei)
    name, rec = the_call(lib)
    assert name == "rlap_approx_chol_from_edges" and nn == NN
    assert (rec["E"], rec["n"], rec["num_remove"], rec["frac"], rec["sym"]) == (E, -1, [-1], 0.5, 1)
    assert (rec["o_v"], rec["o_n"], rec["seed"], rec["perm"], rec["cap"]) == (0, 0, drawn_seed(4), None, 2 * E)
    assert queries(lib) == []   # (no bound is asked for before num_nodes is known)
    check_result(res, rec, 1)
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_from_edges(ei, perm=torch.arange(20))   # an injected perm needs num_nodes
    assert len(exports(lib)) == 1


def test_from_edges_given_num_nodes(lib):
    ei = path(20)
    E = ei.shape[1]
    perm = torch.randperm(20)
    res, nn = ops.approximate_cholesky_from_edges(ei, torch.ones(1, E), 20, 7, "random", "desc", remove_frac=0.25,
                                                  symmetrize=False, perm=perm, seed=3, return_device="meta")
    rec = the_call(lib)[1]
    assert nn == 20 and res.device.type == "meta"
    assert (rec["E"], rec["n"], rec["num_remove"], rec["frac"], rec["sym"], rec["weighted"]) == (E, 20, [7], 0.25, 0, True)
    assert (rec["o_v"], rec["o_n"], rec["seed"], rec["perm"], rec["cap"]) == (0, 1, 3, perm.tolist(), E)
    assert queries(lib) == [(E, 20, 1, 0)]
    ops.approximate_cholesky_from_edges(ei, None, 20, None, "degree", "asc", remove_frac=0.3, mode="frontier")
    rec = exports(lib)[1][1]
    assert (rec["num_remove"], rec["frac"], rec["sym"], rec["cap"]) == ([-1], 0.3, 1, 2 * E)
    assert queries(lib)[1] == (E, 20, 1, 1) and rng_modes(lib) == [0, 1]


def test_batched(lib):
    ei = torch.cat([path(4), path(6) + 4], dim=1)
    E = ei.shape[1]
    perm = torch.cat([torch.randperm(4), torch.randperm(6)])
    sc, ptr = ops.approximate_cholesky_batched(ei, None, [0, 4, 10], torch.tensor([1, 3]), "random", "asc", perm=perm, seed=6)
    name, rec = the_call(lib)
    assert name == "rlap_approx_chol_batched"
    assert (rec["E"], rec["n"], rec["G"], rec["K"], rec["D"]) == (E, 10, 2, 1, 0)
    assert (rec["node_ptr"], rec["num_remove"], rec["perm"], rec["seed"], rec["cap"]) == ([0, 4, 10], [1, 3], perm.tolist(), 6, E)
    assert queries(lib) == [(E, 10, 2, 0)]
    assert ptr.tolist() == [0, 1, 2] and ptr.device.type == "cpu"
    check_result(sc, rec, 2)
    torch.manual_seed(2)
    ops.approximate_cholesky_batched(ei, None, (0, 4, 10), (2, 2), "degree", "asc")
    assert exports(lib)[1][1]["seed"] == 0 and untouched_rng(2)
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_batched(ei, None, [0, 4, 10], [1, 3, 5], "degree", "asc")
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_batched(ei, None, [0, 4, 10], [1, 3], "random", "asc", perm=perm[:9])
    assert len(exports(lib)) == 2


def test_views(lib):
    ei = path(10)
    E = ei.shape[1]
    sc, ptr = ops.approximate_cholesky_views(ei, None, 10, 4, "degree", "asc")
    name, rec = the_call(lib)
    assert name == "rlap_approx_chol_views"
    assert (rec["E"], rec["n"], rec["G"], rec["K"], rec["D"], rec["node_ptr"], rec["num_remove"]) == (E, 10, 1, 1, 0, [0, 10], [4])
    assert (rec["seed"], rec["perm"], rec["cap"]) == (0, None, E) and ptr.tolist() == [0, 1]
    check_result(sc, rec, 1)
    perm = torch.cat([torch.randperm(10) for _ in range(3)])
    torch.manual_seed(9)
    sc, ptr = ops.approximate_cholesky_views(ei, None, 10, [2, 5, 5], "random", "asc", perm=perm)
    rec = exports(lib)[1][1]
    assert (rec["G"], rec["K"], rec["node_ptr"], rec["num_remove"]) == (1, 3, [0, 10], [2, 5, 5])
    assert (rec["perm"], rec["seed"], rec["cap"]) == (perm.tolist(), drawn_seed(9), 3 * E)
    assert ptr.tolist() == [0, 1, 2, 3]
    check_result(sc, rec, 3)
    assert queries(lib) == [(E, 10, 1, 0), (3 * E, 30, 3, 0)]


def test_views_of_a_batch(lib):
    ei = torch.cat([path(4), path(6) + 4], dim=1)
    E = ei.shape[1]
    sc, ptr = ops.approximate_cholesky_views(ei, None, 10, [[1, 2], [3, 4]], "degree", "random", node_ptr=[0, 4, 10], seed=1,
                                             return_device="meta")
    rec = the_call(lib)[1]
    assert (rec["n"], rec["G"], rec["K"], rec["node_ptr"], rec["num_remove"]) == (10, 2, 2, [0, 4, 10], [1, 2, 3, 4])
    assert (rec["o_n"], rec["seed"], rec["cap"]) == (2, 1, 2 * E) and queries(lib) == [(2 * E, 20, 4, 0)]
    assert ptr.tolist() == [0, 1, 2, 3, 4] and sc.device.type == "meta"
    ops.approximate_cholesky_views(ei, None, 10, [3, 5], "degree", "asc", node_ptr=[0, 4, 10])
    assert exports(lib)[1][1]["num_remove"] == [3, 3, 5, 5]
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_views(ei, None, 10, [], "degree", "asc")   # K = 0
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_views(ei, None, 10, [1, 2], "random", "asc", perm=torch.arange(10))   # K * n entries
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_views(ei, None, 11, [1, 2], "degree", "asc", node_ptr=[0, 4, 10])
    assert len(exports(lib)) == 2


def test_depths_of_one_graph(lib):
    ei = path(10)
    E = ei.shape[1]
    perm = torch.randperm(10)
    sc, ptr = ops.approximate_cholesky_depths(ei, None, 10, [1, 3, 3, 8], "random", "asc", perm=perm, seed=4)
    name, rec = the_call(lib)
    assert name == "rlap_approx_chol_depths"
    assert (rec["E"], rec["n"], rec["G"], rec["K"], rec["D"], rec["num_remove"]) == (E, 10, 1, 1, 4, [1, 3, 3, 8])
    assert (rec["perm"], rec["seed"], rec["cap"]) == (perm.tolist(), 4, 4 * E)
    assert queries(lib) == [(E, 10, 1, 0)] and ptr.tolist() == [0, 1, 2, 3, 4]
    check_result(sc, rec, 4)
    ops.approximate_cholesky_depths(ei, None, 10, torch.tensor([2, 6]), "degree", "asc", return_device="meta")
    name, rec = exports(lib)[1]
    assert name == "rlap_approx_chol_depths" and (rec["D"], rec["num_remove"], rec["cap"]) == (2, [2, 6], 2 * E)


def test_depths_of_views_and_batches(lib):
    ei = torch.cat([path(4), path(6) + 4], dim=1)
    E = ei.shape[1]
    perm = torch.cat([torch.randperm(10) for _ in range(2)])
    torch.manual_seed(12)
    sc, ptr = ops.approximate_cholesky_depths(ei, None, 10, [1, 3, 5], "random", "asc", views=2, perm=perm)
    name, rec = the_call(lib)
    assert name == "rlap_approx_chol_views_depths"
    assert (rec["E"], rec["n"], rec["G"], rec["K"], rec["D"], rec["node_ptr"]) == (E, 10, 1, 2, 3, [0, 10])
    assert (rec["num_remove"], rec["perm"], rec["seed"], rec["cap"]) == ([1, 1, 3, 3, 5, 5], perm.tolist(), drawn_seed(12), 6 * E)
    assert queries(lib) == [(2 * E, 20, 2, 0)] and ptr.tolist() == list(range(7))
    check_result(sc, rec, 6)
    ops.approximate_cholesky_depths(ei, None, 10, [2, 4], "degree", "asc", node_ptr=[0, 4, 10])
    name, rec = exports(lib)[1]
    assert name == "rlap_approx_chol_views_depths"
    assert (rec["G"], rec["K"], rec["D"], rec["node_ptr"], rec["num_remove"], rec["cap"]) == (2, 1, 2, [0, 4, 10], [2, 2, 4, 4], 2 * E)
    assert queries(lib)[1] == (E, 10, 2, 0)
    t = [[[1, 2], [0, 3]], [[2, 2], [1, 5]]]   # (D, K, G)
    sc, ptr = ops.approximate_cholesky_depths(ei, None, 10, t, "degree", "random", node_ptr=[0, 4, 10], views=2, seed=7,
                                              return_device="meta")
    name, rec = exports(lib)[2]
    assert (rec["G"], rec["K"], rec["D"], rec["num_remove"], rec["seed"], rec["cap"]) == (2, 2, 2, [1, 2, 0, 3, 2, 2, 1, 5], 7, 4 * E)
    assert queries(lib)[2] == (2 * E, 20, 4, 0) and ptr.tolist() == list(range(9)) and sc.device.type == "meta"
    ops.approximate_cholesky_depths(ei, None, 10, [[[1]], [[2]]], "degree", "asc")   # (D, 1, 1): the views route
    name, rec = exports(lib)[3]
    assert name == "rlap_approx_chol_views_depths" and (rec["G"], rec["K"], rec["D"], rec["num_remove"]) == (1, 1, 2, [1, 2])
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_depths(ei, None, 10, [1, 2], "random", "asc", views=2, perm=torch.arange(10))
    with pytest.raises(AssertionError):
        ops.approximate_cholesky_depths(ei, None, 10, [1, 2], "random", "asc", perm=torch.arange(9))
    assert len(exports(lib)) == 4
