"""The two exports of the symmetric InfoNCE pair (rlap_infonce_pair / rlap_infonce_pair_backward) called through the C ABI on raw
device pointers and a handle of the test's own, after the pattern of tests/test_gpu_infonce_cabi.py: one good call of each against
ops.info_nce_pair; the statuses of the host checks, which answer before anything is launched (the result buffers are filled with a
pattern first and must come back unchanged); a caller's arena that is too small and one of the size the library then asks for."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
RAW = 1
PATTERN = -7.25


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib
    return {"lib": _lib.load(), "_lib": _lib}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def inputs(n=70, f=9):
    g = torch.Generator().manual_seed(n + f)
    a = torch.randn(n, f, generator=g)
    return a.cuda(), (0.3 * a + torch.randn(n, f, generator=g)).cuda()


def forward(env, h, a, b, tau, flags, over=None):
    n, f = a.shape
    out = {k: torch.full((m,), PATTERN, dtype=torch.float64, device="cuda") for k, m in (("loss", 1), ("rows", 2 * n), ("z", 2 * n))}
    info = env["_lib"].InfoncePairInfo()
    c = {"a": ptr(a), "b": ptr(b), "N": n, "F": f, "tau": tau, "flags": flags, "loss": ptr(out["loss"]), "rows": ptr(out["rows"]), "z": ptr(out["z"])}
    c.update(over or {})
    rc = env["lib"].rlap_infonce_pair(h, c["a"], c["b"], c["N"], c["F"], c["tau"], c["flags"], c["loss"], c["rows"], c["z"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def backward(env, h, a, b, tau, flags, z, g, over=None):
    n, f = a.shape
    out = {k: torch.full((n, f), PATTERN, dtype=torch.float32, device="cuda") for k in ("ga", "gb")}
    info = env["_lib"].InfoncePairInfo()
    c = {"a": ptr(a), "b": ptr(b), "N": n, "F": f, "tau": tau, "flags": flags, "z": ptr(z), "g": ptr(g), "ga": ptr(out["ga"]), "gb": ptr(out["gb"])}
    c.update(over or {})
    rc = env["lib"].rlap_infonce_pair_backward(h, c["a"], c["b"], c["N"], c["F"], c["tau"], c["flags"], c["z"], c["g"], c["ga"], c["gb"],
                                               ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def untouched(out):
    return all(bool((t == PATTERN).all()) for t in out.values())


@pytest.mark.parametrize("flags,positive", [(0, "scaled"), (RAW, "raw")])
def test_both_exports_on_raw_pointers(env, handle, flags, positive):
    from rlap_amd import ops
    a, b = inputs()
    rc, out, info = forward(env, handle, a, b, 0.4, flags)
    assert rc == OK and (info.rows, info.features, info.parts, info.groups, info.host_syncs) == (70, 9, 3, 1, 0) and info.arena_bytes > 0
    ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss, rows = ops.info_nce_pair(ta, tb, tau=0.4, positive=positive, return_rows=True)
    assert torch.equal(out["loss"][0], loss.detach()) and torch.equal(out["rows"].view(2, 70), rows)
    g = torch.tensor([1.5], dtype=torch.float64, device="cuda")
    rc, grads, info = backward(env, handle, a, b, 0.4, flags, out["z"], g)
    assert rc == OK and info.host_syncs == 0 and info.rows == 70
    (1.5 * loss).backward()
    assert torch.equal(grads["ga"], ta.grad) and torch.equal(grads["gb"], tb.grad)


def test_host_checks_answer_before_anything_is_launched(env, handle):
    a, b = inputs()
    z = torch.ones(140, dtype=torch.float64, device="cuda")
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    nan = float("nan")
    shared = [
        ({"tau": 0.0}, BAD_ARG), ({"tau": 0.03}, BAD_ARG), ({"tau": 1024.5}, BAD_ARG), ({"tau": -0.4}, BAD_ARG), ({"tau": nan}, BAD_ARG),
        ({"F": 0}, BAD_ARG), ({"N": 0}, BAD_ARG), ({"N": -1}, BAD_ARG), ({"a": None}, BAD_ARG), ({"b": None}, BAD_ARG),
        ({"flags": 2}, BAD_ARG), ({"flags": 1 << 20}, BAD_ARG),
        ({"F": 513}, TOO_LARGE), ({"N": 1 << 31}, TOO_LARGE),
    ]
    for over, want in shared + [({"loss": None}, BAD_ARG), ({"rows": None}, BAD_ARG), ({"z": None}, BAD_ARG)]:
        rc, out, _ = forward(env, handle, a, b, 0.4, 0, over=over)
        assert rc == want and untouched(out), over
    for over, want in shared + [({"z": None}, BAD_ARG), ({"g": None}, BAD_ARG), ({"ga": None}, BAD_ARG), ({"gb": None}, BAD_ARG)]:
        rc, out, _ = backward(env, handle, a, b, 0.4, 0, z, g, over=over)
        assert rc == want and untouched(out), over
    info = env["_lib"].InfoncePairInfo()
    assert env["lib"].rlap_infonce_pair(None, ptr(a), ptr(b), 70, 9, 0.4, 0, ptr(z), ptr(z), ptr(z), ctypes.byref(info)) == BAD_ARG
    for tau in (1.0 / 32.0, 1024.0):                                  # the ends of the range are inside
        assert forward(env, handle, a, b, tau, 0)[0] == OK


def test_a_callers_arena(env, handle):
    lib = env["lib"]
    a, b = inputs()
    base = forward(env, handle, a, b, 0.4, RAW)[1]
    tiny = torch.empty(64, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, _ = forward(env, handle, a, b, 0.4, RAW)
    assert rc == E_WORKSPACE and untouched(out)
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, info = forward(env, handle, a, b, 0.4, RAW)
    assert rc == OK and info.arena_bytes == need.value and all(torch.equal(out[k], base[k]) for k in base)
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    rc, grads, _ = backward(env, handle, a, b, 0.4, RAW, out["z"], g)
    assert rc == E_WORKSPACE and untouched(grads)                      # the backward call needs more: both images of both inputs
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > ws.numel()
    ws2 = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws2.data_ptr(), ws2.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, info = backward(env, handle, a, b, 0.4, RAW, out["z"], g)
    assert rc == OK and info.arena_bytes == need.value and bool(torch.isfinite(grads["ga"]).all()) and not untouched(grads)
