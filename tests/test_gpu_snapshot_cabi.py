"""The five snapshot exports called through the C ABI on a handle of the test's own (rlap_create): the arena the library owns, a
caller's arena that is too small, one of exactly the size the library asks for -- the Python layer always installs its own, so the
first of the three runs nowhere else -- and the statuses of the argument checks, which answer before anything is launched."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

N = 64                 # num_nodes
S = 2                  # two views
F = 4                  # feature columns of the propagation
PPR_CAP = 2 * N * N    # every pair of every segment
MAX_ITER = 64
NAMES = ["stats", "ppr", "subgraph", "gcn_norm", "propagate"]
BAD_ARG, TOO_LARGE, E_WORKSPACE = 3, 9, 11
UNKNOWN_FLAG = 1 << 20
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib, graphs, ops
    sc, ptr = ops.approximate_cholesky_views(graphs.barabasi_albert(N, 3, 1), None, N, [16, 16], "degree", "asc")
    assert ptr.numel() == S + 1 and sc.is_cuda
    x = torch.arange(N * F, dtype=torch.float64, device=sc.device).reshape(N, F)
    ppr, pptr = ops.snapshot_ppr(sc, ptr, N)
    st = ops.snapshot_stats(sc, ptr, N, max_iter=MAX_ITER)
    ei, val, eptr = ops.snapshot_gcn_norm(sc, ptr, N)
    expected = {
        "stats": [st["nodes"], st["lambda_max"], st["iters"], st["converged"]],
        "ppr": [ppr, pptr],
        "subgraph": list(ops.snapshot_subgraph(sc, ptr, N)),
        "gcn_norm": [ei[0], ei[1], val, eptr],
        "propagate": [ops.snapshot_propagate(sc, ptr, N, x)],
    }
    torch.cuda.synchronize()
    return {"lib": _lib.load(), "_lib": _lib, "sc": sc.contiguous(), "ptr": ptr.to(sc.device), "x": x, "expected": expected}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def addr(t):
    return t.data_ptr() if t is not None and t.numel() else None


def call(env, h, name, **over):
    """One export on the test's input, `over` replacing arguments; returns (status, info, outputs trimmed as ops trims them)."""
    lib, _lib, sc, dev = env["lib"], env["_lib"], env["sc"], env["sc"].device
    m = over.get("m", sc.shape[0])
    ptr = over.get("ptr", env["ptr"])
    node_ptr = over.get("node_ptr")
    head = (h, addr(sc) if m else None, m, ptr.data_ptr(), over.get("S", S), addr(node_ptr), over.get("G", 1), over.get("n", N))
    new = lambda *shape, dtype=torch.int64: torch.empty(shape, dtype=dtype, device=dev)
    if name == "stats":
        info = _lib.SnapshotInfo()
        nodes, lam, iters, conv = new(S), new(S, dtype=torch.float64), new(S, dtype=torch.int32), new(S, dtype=torch.int32)
        rc = lib.rlap_snapshot_stats(*head, 0, 1e-10, MAX_ITER, addr(nodes), addr(lam), addr(iters), addr(conv), ctypes.byref(info))
        outs = lambda: [nodes, lam, iters, conv.bool()]
    elif name == "ppr":
        info = _lib.PprInfo()
        out, out_ptr = new(PPR_CAP, 3, dtype=torch.float64), new(S + 1)
        flags = over.get("flags", _lib.PPR_WEIGHTED | _lib.PPR_NORMALIZE)
        rc = lib.rlap_snapshot_ppr(*head, 0.2, 1e-4, 1e-10, flags, addr(out), PPR_CAP, addr(out_ptr), ctypes.byref(info))
        outs = lambda: [out[:info.rows_needed], out_ptr]
    elif name == "subgraph":
        info = _lib.SubgraphInfo()
        cap = min(2 * m, S * N)
        out, out_ptr, ids, ids_ptr = new(m, 3, dtype=torch.float64), new(S + 1), new(cap), new(S + 1)
        rc = lib.rlap_snapshot_subgraph(*head, None, None, 0, over.get("flags", 0), addr(out), addr(out_ptr), addr(ids), cap, addr(ids_ptr),
                                        ctypes.byref(info))
        outs = lambda: [out[:info.rows_kept], out_ptr, ids[:info.ids_written], ids_ptr]
    elif name == "gcn_norm":
        info = _lib.GcnInfo()
        cap = over.get("cap", m + S * N)
        src, dst, val, eptr = new(m + S * N), new(m + S * N), new(m + S * N, dtype=torch.float32), new(S + 1)
        flags = over.get("flags", _lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE | _lib.GCN_F32)
        rc = lib.rlap_snapshot_gcn_norm(*head, flags, 1.0, addr(src), addr(dst), addr(val), cap, addr(eptr), ctypes.byref(info))
        outs = lambda: [src[:info.entries], dst[:info.entries], val[:info.entries], eptr]
    else:
        info = _lib.SpmmInfo()
        y = new(S, N, F, dtype=torch.float64)
        flags = over.get("flags", _lib.GCN_SELF_LOOPS | _lib.GCN_NORMALIZE)
        rc = lib.rlap_snapshot_propagate(*head, flags, 1.0, addr(env["x"]), over.get("F", F), addr(y), ctypes.byref(info))
        outs = lambda: [y]
    torch.cuda.synchronize()
    return rc, info, (outs() if rc == 0 else None)


def same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, w.dtype, tuple(g.shape), tuple(w.shape))
        if g.dtype.is_floating_point:
            bits = torch.int64 if g.dtype == torch.float64 else torch.int32
            g, w = g.contiguous().view(bits), w.contiguous().view(bits)
        assert torch.equal(g, w)


@pytest.mark.parametrize("name", NAMES)
def test_owned_arena_short_arena_exact_arena(env, handle, name):
    lib, dev = env["lib"], env["sc"].device
    # the library's own arena
    rc, info, outs = call(env, handle, name)
    assert rc == 0
    same_bits(outs, env["expected"][name])
    # a caller's arena of 256 bytes: refused, and the size it takes reported
    short = torch.empty(256, dtype=torch.uint8, device=dev)
    assert lib.rlap_set_workspace(handle, short.data_ptr(), 256, None, 0) == 0
    rc, _, _ = call(env, handle, name)
    assert rc == E_WORKSPACE
    need, rng = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rng)) == 0
    assert need.value > 256
    # exactly that size
    exact = torch.empty(need.value, dtype=torch.uint8, device=dev)
    assert lib.rlap_set_workspace(handle, exact.data_ptr(), need.value, None, 0) == 0
    rc, info, outs = call(env, handle, name)
    assert rc == 0
    same_bits(outs, env["expected"][name])
    if name != "stats":   # (rlap_snapshot_info reports no arena size)
        assert info.arena_bytes == need.value


FLAGGED = ["ppr", "subgraph", "gcn_norm", "propagate"]   # (rlap_snapshot_stats has no flags and no limit on num_nodes)
STATUS_TABLE = (
    [(name, dict(S=0), BAD_ARG) for name in NAMES if name != "subgraph"]
    + [(name, dict(flags=UNKNOWN_FLAG), BAD_ARG) for name in FLAGGED]
    + [(name, dict(G=3, node_ptr=[0, 20, 40, N]), BAD_ARG) for name in NAMES]
    + [(name, dict(n=INT32_MAX), TOO_LARGE) for name in FLAGGED]
    + [(name, dict(flags=UNKNOWN_FLAG, n=INT32_MAX), BAD_ARG) for name in FLAGGED]
    + [("gcn_norm", dict(cap=0, n=INT32_MAX), TOO_LARGE), ("propagate", dict(F=0), BAD_ARG)]
)


def test_statuses_of_the_argument_checks(env, handle):
    """Every input is an honest one that the call refuses before its first launch."""
    dev = env["sc"].device
    for name, over, status in STATUS_TABLE:
        if "node_ptr" in over:
            over = dict(over, node_ptr=torch.tensor(over["node_ptr"], dtype=torch.int64, device=dev))
        rc, _, _ = call(env, handle, name, **over)
        assert rc == status, (name, over, rc)
    # no segment at all is a call that the subgraph export alone accepts: no rows, no ids, one offset each
    rc, info, outs = call(env, handle, "subgraph", S=0, m=0, ptr=torch.zeros(1, dtype=torch.int64, device=dev))
    assert rc == 0 and (info.rows_kept, info.ids_written) == (0, 0)
    assert outs[0].numel() == 0 and outs[2].numel() == 0 and int(outs[1][0]) == 0 and int(outs[3][0]) == 0


E_OUT_CAPACITY = 13
POISON = 0x7FF8DEADBEEF1234   # a quiet NaN no call computes


def test_ppr_output_capacity_one_short_then_exact(env, handle):
    """rlap_snapshot_ppr with room for one row less than it keeps: status 13, the exact count reported, d_out and d_out_ptr left as
    they were; with exactly that many rows: the expected bits."""
    lib, _lib, sc, dev = env["lib"], env["_lib"], env["sc"], env["sc"].device
    want, want_ptr = env["expected"]["ppr"]
    rows = want.shape[0]
    assert rows > 1 and rows < PPR_CAP
    assert _lib.E_OUT_CAPACITY == E_OUT_CAPACITY
    for cap, status in [(rows - 1, E_OUT_CAPACITY), (0, E_OUT_CAPACITY), (rows, 0)]:
        out = torch.full((rows, 3), POISON, dtype=torch.int64, device=dev)
        out_ptr = torch.full((S + 1,), POISON, dtype=torch.int64, device=dev)
        info = _lib.PprInfo()
        rc = lib.rlap_snapshot_ppr(handle, addr(sc), sc.shape[0], env["ptr"].data_ptr(), S, None, 1, N, 0.2, 1e-4, 1e-10,
                                   _lib.PPR_WEIGHTED | _lib.PPR_NORMALIZE, addr(out), cap, addr(out_ptr), ctypes.byref(info))
        torch.cuda.synchronize()
        assert rc == status, (cap, rc)
        assert info.rows_needed == rows and info.steps == 35
        if status:
            assert bool((out == POISON).all()) and bool((out_ptr == POISON).all()), "a refused call wrote to its outputs"
        else:
            same_bits([out.view(torch.float64), out_ptr], [want, want_ptr])
