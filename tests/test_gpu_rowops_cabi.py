"""The four row-pass exports (rlap_bias_act_dropout, rlap_layer_norm and their _backward calls) called through the C ABI on raw device
pointers and a handle of the test's own, after the pattern of tests/test_gpu_norm_cabi.py: one good call of each against the host
mirror; the statuses of the host checks, which answer before anything is launched (the result buffers are filled with a pattern
first and must come back unchanged); null gradient outputs, which are skipped; the arena at exactly its stated size, a caller's
that is too small and one of the size the library then asks for."""
import ctypes

import numpy as np
import pytest
import torch

import rowops_mirror as rm

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
PATTERN = -7.25
L, N, F = 2, 300, 12
P, SEED = 0.25, 2 ** 63 + 5
FLAGS = rm.ACT_PRELU | rm.SLOPE_PER_CHANNEL | rm.TRAINING


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib
    return {"lib": _lib.load(), "_lib": _lib}


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return rm.build(tmp_path_factory.mktemp("rowops"))


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
    d = rm.inputs(L, N, F, 21)
    return d, {k: torch.from_numpy(v).cuda() for k, v in d.items()}


def call(env, h, t, which, backward, flags=FLAGS, over=None):
    """One export: (status, its outputs pre-filled with the pattern, the info struct)."""
    ln = which == "layer_norm"
    out = {("gx" if backward else "y"): torch.full((L, N, F), PATTERN, dtype=torch.float32, device="cuda")}
    if backward:
        out.update({k: torch.full((F,), PATTERN, dtype=torch.float32, device="cuda") for k in (("gweight",) if ln else ()) + ("gbias", "gslope")})
    info = env["_lib"].RowopsInfo()
    c = {"x": ptr(t["x"]), "gy": ptr(t["gy"]), "L": L, "N": N, "F": F, "weight": ptr(t["weight"]), "bias": ptr(t["bias"]), "slope": ptr(t["slope"]),
         "eps": 1e-5, "p": P, "seed": SEED, "flags": flags}
    c.update({k: ptr(v) for k, v in out.items()})
    c.update(over or {})
    head = [c["x"]] + ([c["gy"]] if backward else []) + [c["L"], c["N"], c["F"]] + ([c["weight"]] if ln else []) + [c["bias"], c["slope"]]
    head += ([c["eps"]] if ln else []) + [c["p"], c["seed"], c["flags"]]
    tail = [c["gx"]] + ([c["gweight"]] if ln else []) + [c["gbias"], c["gslope"]] if backward else [c["y"]]
    name = ("rlap_layer_norm" if ln else "rlap_bias_act_dropout") + ("_backward" if backward else "")
    rc = getattr(env["lib"], name)(h, *head, *tail, ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def untouched(out):
    return all(bool((t == PATTERN).all()) for t in out.values())


def bits(t):
    return t.cpu().numpy().tobytes()


def test_the_four_exports_on_raw_pointers(env, handle, mirror):
    d, t = inputs()
    rc, out, info = call(env, handle, t, "epilogue", False)
    assert rc == OK and (info.rows, info.features, info.layers, info.chunks, info.vec, info.launches, info.instance, info.host_syncs) == (N, F, L, 2, 1, 1, 0, 0)
    assert info.arena_bytes == 0
    assert bits(out["y"]) == rm.forward(mirror, d["x"], d["bias"], d["slope"], P, SEED, FLAGS).tobytes()
    rc, grads, info = call(env, handle, t, "epilogue", True)
    assert rc == OK and (info.vec, info.launches, info.host_syncs) == (1, 3, 0)
    assert info.arena_bytes == mirror.rowops_backward_bytes(L, N, F, 1, 1) > 0                  # the arena at exactly its stated size
    m = rm.backward(mirror, d["x"], d["gy"], d["bias"], d["slope"], P, SEED, FLAGS)
    assert all(bits(grads[k]) == m[k].tobytes() for k in ("gx", "gbias", "gslope"))
    rc, out, info = call(env, handle, t, "layer_norm", False)
    assert rc == OK and (info.vec, info.launches, info.instance, info.arena_bytes) == (1, 1, 1, 0)
    assert bits(out["y"]) == rm.ln_forward(mirror, d["x"], d["weight"], d["bias"], d["slope"], 1e-5, P, SEED, FLAGS)[0].tobytes()
    rc, grads, info = call(env, handle, t, "layer_norm", True)
    assert rc == OK and (info.vec, info.launches, info.instance, info.host_syncs) == (1, 4, 1, 0)
    assert info.arena_bytes == mirror.rowops_ln_backward_bytes(L, N, F, 1, 1, 1)
    m = rm.ln_backward(mirror, d["x"], d["gy"], d["weight"], d["bias"], d["slope"], 1e-5, P, SEED, FLAGS)
    assert all(bits(grads[k]) == m[k].tobytes() for k in ("gx", "gweight", "gbias", "gslope"))


@pytest.mark.parametrize("which", ["epilogue", "layer_norm"])
def test_the_single_slope_is_one_value_and_no_slope_is_none(env, handle, which):
    _, t = inputs()
    rc, grads, _ = call(env, handle, t, which, True, flags=rm.ACT_PRELU | rm.TRAINING)
    assert rc == OK and bool((grads["gslope"][1:] == PATTERN).all()) and float(grads["gslope"][0]) != PATTERN
    rc, grads, _ = call(env, handle, t, which, True, flags=rm.ACT_RELU | rm.TRAINING)
    assert rc == OK and bool((grads["gslope"] == PATTERN).all()) and not untouched({"gx": grads["gx"]})   # (ignored without PReLU)


@pytest.mark.parametrize("which", ["epilogue", "layer_norm"])
def test_null_gradient_outputs_are_skipped(env, handle, which):
    _, t = inputs()
    rc, full, info = call(env, handle, t, which, True)
    with_params = info.launches
    assert rc == OK and with_params == (4 if which == "layer_norm" else 3)
    for skip in full:
        rc, part, info = call(env, handle, t, which, True, over={skip: None})
        assert rc == OK and bool((part[skip] == PATTERN).all()) and info.launches == with_params
        assert all(torch.equal(part[k], full[k]) for k in full if k != skip), skip
    params = {k: None for k in full if k != "gx"}
    rc, part, info = call(env, handle, t, which, True, over=params)
    assert rc == OK and info.launches == 1 and info.arena_bytes == 0 and torch.equal(part["gx"], full["gx"])   # the one pass alone
    rc, part, info = call(env, handle, t, which, True, over=dict(params, gx=None))
    assert rc == OK and info.launches == 0 and untouched(part)


@pytest.mark.parametrize("which", ["epilogue", "layer_norm"])
def test_host_checks_answer_before_anything_is_launched(env, handle, which):
    _, t = inputs()
    shared = [
        ({"flags": rm.ACT_RELU | rm.ACT_PRELU}, BAD_ARG), ({"flags": rm.ACT_PRELU, "slope": None}, BAD_ARG), ({"flags": rm.SLOPE_PER_CHANNEL}, BAD_ARG),
        ({"N": 0}, BAD_ARG), ({"F": 0}, BAD_ARG), ({"F": 4097}, BAD_ARG), ({"L": 0}, BAD_ARG), ({"p": -0.1}, BAD_ARG), ({"p": 1.0}, BAD_ARG),
        ({"p": float("nan")}, BAD_ARG), ({"x": None}, BAD_ARG), ({"flags": 16}, BAD_ARG), ({"L": 1 << 30, "N": 1 << 20}, TOO_LARGE),
    ]
    if which == "layer_norm":
        shared += [({"eps": 0.0}, BAD_ARG), ({"eps": float("nan")}, BAD_ARG), ({"eps": float("inf")}, BAD_ARG)]
    for over, want in shared + [({"y": None}, BAD_ARG)]:
        rc, out, _ = call(env, handle, t, which, False, over=over)
        assert rc == want and untouched(out), over
    for over, want in shared + [({"gy": None}, BAD_ARG)]:
        rc, out, _ = call(env, handle, t, which, True, over=over)
        assert rc == want and untouched(out), over
    assert call(env, None, t, which, False)[0] == BAD_ARG
    assert call(env, handle, t, which, False, over={"N": 1, "p": 0.0})[0] == OK and call(env, handle, t, which, False, over={"p": 0.999999})[0] == OK


@pytest.mark.parametrize("which", ["epilogue", "layer_norm"])
def test_a_callers_arena(env, handle, which):
    lib = env["lib"]
    _, t = inputs()
    base = call(env, handle, t, which, True)[1]
    tiny = torch.empty(64, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, info = call(env, handle, t, which, False)
    assert rc == OK and info.arena_bytes == 0 and not untouched(out)              # the forward calls take no scratch
    rc, grads, _ = call(env, handle, t, which, True)
    assert rc == E_WORKSPACE and untouched(grads)
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, info = call(env, handle, t, which, True)
    assert rc == OK and info.arena_bytes == need.value and all(torch.equal(grads[k], base[k]) for k in base)
