"""rlap_snapshot_markov called through the C ABI on a handle of the test's own (rlap_create): RLAP_E_OUT_CAPACITY with the count and
nothing written, RLAP_E_WORKSPACE on a short arena and the call on an arena of exactly the size asked for, RLAP_E_BAD_ARG for every
parameter rule, and the empty inputs S = 0 and m = 0."""
import ctypes

import numpy as np
import pytest
import torch

import markov_mirror as mm
from util import ba_graph

pytestmark = pytest.mark.gpu

N = 150
OK, BAD_ARG, E_WORKSPACE, E_OUT_CAPACITY = 0, 3, 11, 13


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib, ops
    parts = []
    for s, n in enumerate((N, 40)):
        ei = np.asarray(ba_graph(n, 3, s + 1))
        parts.append(mm.column_layout(ei, mm.symmetric_weights(ei, s)))
    sc = torch.from_numpy(np.concatenate(parts)).cuda()
    ptr = torch.tensor([0, parts[0].shape[0], sc.shape[0]], dtype=torch.int64)
    out, mptr = ops.snapshot_markov(sc, ptr, N, order=4, eps=1e-3)
    torch.cuda.synchronize()
    return {"lib": _lib.load(), "_lib": _lib, "sc": sc, "ptr": ptr.cuda(), "out": out, "mptr": mptr}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def call(env, h, cap=None, **over):
    """One call on the test's input, `over` replacing arguments: (status, info, out buffer, out_ptr buffer)."""
    lib, _lib, sc = env["lib"], env["_lib"], over.get("sc", env["sc"])
    dev = env["sc"].device
    m = over.get("m", sc.shape[0])
    S = over.get("S", 2)
    cap = env["out"].shape[0] if cap is None else cap
    out = torch.full((max(cap, 1), 3), -7.0, dtype=torch.float64, device=dev)
    out_ptr = torch.full((S + 1,), -7, dtype=torch.int64, device=dev)
    info = _lib.MarkovInfo()
    ptr = over.get("ptr", env["ptr"])
    rc = lib.rlap_snapshot_markov(h, sc.data_ptr() if m else None, m, ptr.data_ptr(), S, None, 1, over.get("n", N), over.get("alpha", 0.2),
                                  over.get("order", 4), over.get("eps", 1e-3), over.get("flags", _lib.MARKOV_WEIGHTED | _lib.MARKOV_SELF_LOOP),
                                  out.data_ptr() if cap else None, cap, out_ptr.data_ptr(), ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, info, out, out_ptr


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def test_the_call_and_its_report(env, handle):
    rc, info, out, out_ptr = call(env, handle)
    P = env["out"].shape[0]
    assert rc == OK and info.rows_needed == P and same_bits(out[:P], env["out"]) and torch.equal(out_ptr, env["mptr"])
    assert (info.order, info.small_tiles, info.large_tiles, info.groups, info.host_syncs) == (4, 4, 0, 1, 3)
    assert info.launches == 2 + 4 and info.arena_bytes > 0


def test_out_capacity_reports_the_count_and_writes_nothing(env, handle):
    P = env["out"].shape[0]
    for cap in (P - 1, 1, 0):
        rc, info, out, out_ptr = call(env, handle, cap=cap)
        assert rc == E_OUT_CAPACITY and info.rows_needed == P
        assert bool((out == -7.0).all()) and bool((out_ptr == -7).all())
    rc, info, out, _ = call(env, handle, cap=P)
    assert rc == OK and same_bits(out[:P], env["out"])


def test_short_arena_then_exact_arena(env, handle):
    lib, dev = env["lib"], env["sc"].device
    short = torch.empty(256, dtype=torch.uint8, device=dev)
    assert lib.rlap_set_workspace(handle, short.data_ptr(), 256, None, 0) == 0
    rc, _, out, _ = call(env, handle)
    assert rc == E_WORKSPACE and bool((out == -7.0).all())
    need, rng = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rng)) == 0 and need.value > 256
    exact = torch.empty(need.value, dtype=torch.uint8, device=dev)
    assert lib.rlap_set_workspace(handle, exact.data_ptr(), need.value, None, 0) == 0
    rc, info, out, out_ptr = call(env, handle)
    P = env["out"].shape[0]
    assert rc == OK and info.arena_bytes == need.value and same_bits(out[:P], env["out"]) and torch.equal(out_ptr, env["mptr"])


def test_bad_arguments(env, handle):
    _lib = env["_lib"]
    for over in (dict(alpha=-1e-9), dict(alpha=1.0000001), dict(alpha=float("nan")), dict(order=0), dict(order=-1),
                 dict(order=_lib.MARKOV_MAX_ORDER + 1), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("inf")), dict(eps=float("nan")),
                 dict(flags=1 << 20), dict(flags=16), dict(S=0)):
        rc, info, out, _ = call(env, handle, **over)
        assert rc == BAD_ARG and bool((out == -7.0).all()), over
    for over in (dict(alpha=0.0), dict(alpha=1.0), dict(order=1), dict(order=_lib.MARKOV_MAX_ORDER, eps=0.5)):
        rc, _, _, _ = call(env, handle, cap=N * N + 40 * 40, **over)
        assert rc == OK, over
    # weights: <= 0 or not finite with RLAP_MARKOV_WEIGHTED; a zero passes with RLAP_MARKOV_ZERO_ROWS, a negative one never;
    # without the weighted flag the column is not read as a weight
    W, L, Z = _lib.MARKOV_WEIGHTED, _lib.MARKOV_SELF_LOOP, _lib.MARKOV_ZERO_ROWS
    for value, flags, want in [(0.0, W | L, BAD_ARG), (-1.0, W | L, BAD_ARG), (float("inf"), W | L, BAD_ARG), (float("nan"), W | L, BAD_ARG),
                               (0.0, W | L | Z, OK), (-1.0, W | L | Z, BAD_ARG), (-1.0, L, OK)]:
        sc = env["sc"].clone()
        sc[3, 2] = value
        rc, _, _, _ = call(env, handle, cap=N * N + 40 * 40, sc=sc, flags=flags)
        assert rc == want, (value, flags)


def test_no_rows(env, handle):
    zeros = torch.zeros(3, dtype=torch.int64, device=env["sc"].device)
    rc, info, out, out_ptr = call(env, handle, m=0, ptr=zeros, cap=0)
    assert rc == OK and info.rows_needed == 0 and out_ptr.tolist() == [0, 0, 0] and info.launches == 0
    rc, info, out, out_ptr = call(env, handle, m=0, ptr=zeros, cap=5)
    assert rc == OK and out_ptr.tolist() == [0, 0, 0] and bool((out == -7.0).all())
