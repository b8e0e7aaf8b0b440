"""The two batch norm exports (rlap_batch_norm / rlap_batch_norm_backward) called through the C ABI on raw device pointers and a handle
of the test's own, after the pattern of tests/test_gpu_cca_cabi.py: one good call of each against ops.batch_norm; the statuses of the
host checks, which answer before anything is launched (the result buffers are filled with a pattern first and must come back
unchanged); null gradient outputs, which are skipped; the arena at its stated bound, a caller's that is too small and one of the size
the library then asks for."""
import ctypes

import numpy as np
import pytest
import torch

import norm_mirror as nm

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
PATTERN = -7.25
L, N, F = 2, 300, 12


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib
    return {"lib": _lib.load(), "_lib": _lib}


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return nm.build(tmp_path_factory.mktemp("norm"))


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def inputs():
    d = nm.inputs(L, N, F, 21)
    return {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def forward(env, h, t, flags=nm.PRE_RELU | nm.POST_PRELU | nm.SLOPE_PER_CHANNEL, over=None):
    out = {"y": torch.full((L, N, F), PATTERN, dtype=torch.float32, device="cuda"),
           "stat": torch.full((L, 3, F), PATTERN, dtype=torch.float64, device="cuda")}
    bufs = {"rm": t["running_mean"].clone(), "rv": t["running_var"].clone()}
    info = env["_lib"].NormInfo()
    c = {"x": ptr(t["x"]), "L": L, "N": N, "F": F, "weight": ptr(t["weight"]), "bias": ptr(t["bias"]), "slope": ptr(t["slope"]), "rm": ptr(bufs["rm"]),
         "rv": ptr(bufs["rv"]), "momentum": 0.1, "eps": 1e-5, "flags": flags, "y": ptr(out["y"]), "stat": ptr(out["stat"])}
    c.update(over or {})
    rc = env["lib"].rlap_batch_norm(h, c["x"], c["L"], c["N"], c["F"], c["weight"], c["bias"], c["slope"], c["rm"], c["rv"], c["momentum"], c["eps"],
                                    c["flags"], c["y"], c["stat"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, bufs, info


def backward(env, h, t, stat, flags=nm.PRE_RELU | nm.POST_PRELU | nm.SLOPE_PER_CHANNEL, over=None):
    out = {"gx": torch.full((L, N, F), PATTERN, dtype=torch.float32, device="cuda")}
    out.update({k: torch.full((F,), PATTERN, dtype=torch.float32, device="cuda") for k in ("gweight", "gbias", "gslope")})
    info = env["_lib"].NormInfo()
    c = {"x": ptr(t["x"]), "gy": ptr(t["gy"]), "L": L, "N": N, "F": F, "weight": ptr(t["weight"]), "bias": ptr(t["bias"]), "slope": ptr(t["slope"]),
         "rm": ptr(t["running_mean"]), "rv": ptr(t["running_var"]), "eps": 1e-5, "flags": flags, "stat": ptr(stat)}
    c.update({k: ptr(v) for k, v in out.items()})
    c.update(over or {})
    rc = env["lib"].rlap_batch_norm_backward(h, c["x"], c["gy"], c["L"], c["N"], c["F"], c["weight"], c["bias"], c["slope"], c["rm"], c["rv"], c["eps"],
                                             c["flags"], c["stat"], c["gx"], c["gweight"], c["gbias"], c["gslope"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def untouched(out):
    return all(bool((t == PATTERN).all()) for t in out.values())


def test_both_exports_on_raw_pointers(env, handle, mirror):
    from rlap_amd import ops
    t = inputs()
    rc, out, bufs, info = forward(env, handle, t)
    assert rc == OK and (info.rows, info.features, info.layers, info.chunks, info.vec, info.launches, info.host_syncs) == (N, F, L, 2, 1, 3, 0)
    assert info.arena_bytes == mirror.norm_forward_bytes(L, N, F, 0) > 0                      # the arena at its stated bound
    x, w, b, s = (t[k].clone().requires_grad_(True) for k in ("x", "weight", "bias", "slope"))
    rm, rv = t["running_mean"].clone(), t["running_var"].clone()
    y = ops.batch_norm(x, w, b, rm, rv, pre="relu", post="prelu", slope=s)
    assert torch.equal(out["y"], y.detach()) and torch.equal(bufs["rm"], rm) and torch.equal(bufs["rv"], rv)
    assert not torch.equal(rm, t["running_mean"]) and bool(torch.isfinite(out["stat"]).all())
    rc, grads, info = backward(env, handle, t, out["stat"])
    assert rc == OK and (info.vec, info.launches, info.host_syncs) == (1, 3, 0)
    assert info.arena_bytes == mirror.norm_backward_bytes(L, N, F, nm.POST_PRELU)
    y.backward(t["gy"])
    assert torch.equal(grads["gx"], x.grad) and torch.equal(grads["gweight"], w.grad) and torch.equal(grads["gbias"], b.grad)
    assert torch.equal(grads["gslope"], s.grad)


def test_the_single_slope_is_one_value(env, handle):
    t = inputs()
    flags = nm.POST_PRELU
    rc, out, _, _ = forward(env, handle, t, flags=flags)
    rc2, grads, info = backward(env, handle, t, out["stat"], flags=flags)
    assert rc == OK and rc2 == OK and info.launches == 3
    assert bool((grads["gslope"][1:] == PATTERN).all()) and float(grads["gslope"][0]) != PATTERN


def test_null_gradient_outputs_are_skipped(env, handle):
    t = inputs()
    _, out, _, _ = forward(env, handle, t)
    rc, full, _ = backward(env, handle, t, out["stat"])
    assert rc == OK
    for skip in ("gx", "gweight", "gbias", "gslope"):
        rc, part, info = backward(env, handle, t, out["stat"], over={skip: None})
        assert rc == OK and bool((part[skip] == PATTERN).all()) and info.launches == 3
        assert all(torch.equal(part[k], full[k]) for k in full if k != skip), skip
    # evaluation mode: without a parameter gradient the apply pass alone
    rc, part, info = backward(env, handle, t, None, flags=nm.EVAL, over={"gweight": None, "gbias": None, "gslope": None})
    assert rc == OK and info.launches == 1 and not untouched({"gx": part["gx"]})
    rc, withp, info = backward(env, handle, t, None, flags=nm.EVAL)
    assert rc == OK and info.launches == 3 and torch.equal(withp["gx"], part["gx"]) and bool((withp["gslope"] == PATTERN).all())


def test_host_checks_answer_before_anything_is_launched(env, handle):
    t = inputs()
    stat = torch.ones(L, 3, F, dtype=torch.float64, device="cuda")
    both = nm.POST_RELU | nm.POST_PRELU
    shared = [
        ({"flags": both}, BAD_ARG), ({"flags": nm.POST_PRELU, "slope": None}, BAD_ARG), ({"flags": nm.EVAL, "rm": None}, BAD_ARG),
        ({"flags": nm.EVAL, "rv": None}, BAD_ARG), ({"N": 1}, BAD_ARG), ({"N": 0, "flags": nm.EVAL}, BAD_ARG), ({"F": 0}, BAD_ARG),
        ({"F": 4097}, BAD_ARG), ({"L": 0}, BAD_ARG), ({"eps": 0.0}, BAD_ARG), ({"eps": float("nan")}, BAD_ARG), ({"eps": float("inf")}, BAD_ARG),
        ({"x": None}, BAD_ARG), ({"flags": 32}, BAD_ARG), ({"stat": None}, BAD_ARG), ({"L": 1 << 30, "N": 1 << 20}, TOO_LARGE),
    ]
    fwd_only = [({"momentum": -0.1}, BAD_ARG), ({"momentum": 1.5}, BAD_ARG), ({"momentum": float("nan")}, BAD_ARG), ({"y": None}, BAD_ARG)]
    for over, want in shared + fwd_only:
        rc, out, bufs, _ = forward(env, handle, t, over=over)
        assert rc == want and untouched(out), over
        assert torch.equal(bufs["rm"], t["running_mean"]) and torch.equal(bufs["rv"], t["running_var"]), over
    for over, want in shared + [({"gy": None}, BAD_ARG)]:
        rc, out, _ = backward(env, handle, t, stat, over=over)
        assert rc == want and untouched(out), over
    info = env["_lib"].NormInfo()
    y = torch.empty(L, N, F, device="cuda")
    assert env["lib"].rlap_batch_norm(None, ptr(t["x"]), L, N, F, None, None, None, None, None, 0.1, 1e-5, 0, ptr(y), ptr(stat), ctypes.byref(info)) == BAD_ARG
    assert forward(env, handle, t, over={"momentum": 0.0, "N": 2})[0] == OK and forward(env, handle, t, over={"momentum": 1.0})[0] == OK
    assert forward(env, handle, t, flags=nm.EVAL, over={"N": 1, "stat": None})[0] == OK       # the ends of the ranges are inside


def test_a_callers_arena(env, handle):
    lib = env["lib"]
    t = inputs()
    base = forward(env, handle, t)[1]
    tiny = torch.empty(64, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, bufs, _ = forward(env, handle, t)
    assert rc == E_WORKSPACE and untouched(out) and torch.equal(bufs["rm"], t["running_mean"])
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, _, info = forward(env, handle, t)
    assert rc == OK and info.arena_bytes == need.value and all(torch.equal(out[k], base[k]) for k in base)
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, _ = backward(env, handle, t, out["stat"])
    assert rc == E_WORKSPACE and untouched(grads)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws2 = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws2.data_ptr(), ws2.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, info = backward(env, handle, t, out["stat"])
    assert rc == OK and info.arena_bytes == need.value and bool(torch.isfinite(grads["gx"]).all()) and not untouched(grads)
