"""The two Barlow Twins exports (rlap_bt_loss / rlap_bt_loss_backward) called through the C ABI on raw device pointers and a handle
of the test's own, after the pattern of tests/test_gpu_cca_cabi.py: one good call of each against ops.barlow_twins_loss; the
statuses of the host checks, which answer before anything is launched (the result buffers are filled with a pattern first and must
come back unchanged); a caller's arena that is too small and one of the size the library then asks for."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
PATTERN = -7.25
EPS = 1e-15


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
    a = torch.randn(n, f, generator=g) + 0.5
    return a.cuda(), (0.6 * a.roll(-1, 1) + 0.4 * torch.randn(n, f, generator=g) + 1.0).cuda()


def forward(env, h, a, b, lambd, flags=0, over=None):
    n, f = a.shape
    out = {"terms": torch.full((3,), PATTERN, dtype=torch.float64, device="cuda"),
           "colstat": torch.full((4 * f,), PATTERN, dtype=torch.float64, device="cuda"),
           "cross": torch.full((f, f), PATTERN, dtype=torch.float32, device="cuda")}
    info = env["_lib"].BtInfo()
    c = {"a": ptr(a), "b": ptr(b), "N": n, "F": f, "lambd": lambd, "eps": EPS, "flags": flags, "terms": ptr(out["terms"]),
         "colstat": ptr(out["colstat"]), "cross": ptr(out["cross"])}
    c.update(over or {})
    rc = env["lib"].rlap_bt_loss(h, c["a"], c["b"], c["N"], c["F"], c["lambd"], c["eps"], c["flags"], c["terms"], c["colstat"], c["cross"],
                                 ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def backward(env, h, a, b, lambd, colstat, cross, g, flags=0, over=None):
    n, f = a.shape
    out = {k: torch.full((n, f), PATTERN, dtype=torch.float32, device="cuda") for k in ("ga", "gb")}
    info = env["_lib"].BtInfo()
    c = {"a": ptr(a), "b": ptr(b), "N": n, "F": f, "lambd": lambd, "eps": EPS, "flags": flags, "colstat": ptr(colstat), "cross": ptr(cross),
         "g": ptr(g), "ga": ptr(out["ga"]), "gb": ptr(out["gb"])}
    c.update(over or {})
    rc = env["lib"].rlap_bt_loss_backward(h, c["a"], c["b"], c["N"], c["F"], c["lambd"], c["eps"], c["flags"], c["colstat"], c["cross"], c["g"],
                                          c["ga"], c["gb"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def untouched(out):
    return all(bool((t == PATTERN).all()) for t in out.values())


@pytest.mark.parametrize("lambd", [1.0 / 9, 0.5])
def test_both_exports_on_raw_pointers(env, handle, lambd):
    from rlap_amd import ops
    a, b = inputs()
    rc, out, info = forward(env, handle, a, b, lambd)
    assert rc == OK and (info.rows, info.features, info.parts, info.host_syncs) == (70, 9, 3, 0) and info.arena_bytes > 0
    ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    terms = ops.barlow_twins_loss(ta, tb, lambd=lambd, return_terms=True)
    assert torch.equal(out["terms"], torch.stack([t.detach() for t in terms]))
    assert bool(torch.isfinite(out["colstat"]).all()) and not torch.equal(out["cross"], out["cross"].t())
    g = torch.tensor([1.5], dtype=torch.float64, device="cuda")
    rc, grads, info = backward(env, handle, a, b, lambd, out["colstat"], out["cross"], g)
    assert rc == OK and info.host_syncs == 0 and info.rows == 70
    (1.5 * terms[0]).backward()
    assert torch.equal(grads["ga"], ta.grad) and torch.equal(grads["gb"], tb.grad)


def test_the_flag_takes_the_inputs_as_they_are_and_needs_no_colstat(env, handle):
    from rlap_amd import ops
    a, b = inputs()
    rc, out, _ = forward(env, handle, a, b, 0.5, flags=1)
    assert rc == OK and bool((out["colstat"] == PATTERN).all())               # not written
    rc, out2, _ = forward(env, handle, a, b, 0.5, flags=1, over={"colstat": None})
    assert rc == OK and torch.equal(out2["terms"], out["terms"]) and torch.equal(out2["cross"], out["cross"])
    ta = a.clone().requires_grad_(True)
    terms = ops.barlow_twins_loss(ta, b, lambd=0.5, standardize=False, return_terms=True)
    assert torch.equal(out["terms"], torch.stack([t.detach() for t in terms]))
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    rc, grads, _ = backward(env, handle, a, b, 0.5, None, out["cross"], g, flags=1)
    terms[0].backward()
    assert rc == OK and torch.equal(grads["ga"], ta.grad)


def test_host_checks_answer_before_anything_is_launched(env, handle):
    a, b = inputs()
    colstat = torch.ones(36, dtype=torch.float64, device="cuda")
    cross = torch.ones(9, 9, dtype=torch.float32, device="cuda")
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    shared = [
        ({"lambd": -1e-3}, BAD_ARG), ({"lambd": float("nan")}, BAD_ARG), ({"lambd": float("inf")}, BAD_ARG),
        ({"eps": -1e-15}, BAD_ARG), ({"eps": float("nan")}, BAD_ARG), ({"eps": float("inf")}, BAD_ARG),
        ({"F": 0}, BAD_ARG), ({"F": 513}, BAD_ARG), ({"N": 1}, BAD_ARG), ({"N": 0}, BAD_ARG), ({"N": -1}, BAD_ARG),
        ({"a": None}, BAD_ARG), ({"b": None}, BAD_ARG), ({"flags": 2}, BAD_ARG), ({"flags": 3}, BAD_ARG), ({"flags": 1 << 20}, BAD_ARG),
        ({"N": 1 << 31}, TOO_LARGE),
    ]
    for over, want in shared + [({"terms": None}, BAD_ARG), ({"colstat": None}, BAD_ARG), ({"cross": None}, BAD_ARG)]:
        rc, out, _ = forward(env, handle, a, b, 0.1, over=over)
        assert rc == want and untouched(out), over
    for over, want in shared + [({"colstat": None}, BAD_ARG), ({"cross": None}, BAD_ARG), ({"g": None}, BAD_ARG), ({"ga": None}, BAD_ARG),
                                ({"gb": None}, BAD_ARG)]:
        rc, out, _ = backward(env, handle, a, b, 0.1, colstat, cross, g, over=over)
        assert rc == want and untouched(out), over
    info = env["_lib"].BtInfo()
    assert env["lib"].rlap_bt_loss(None, ptr(a), ptr(b), 70, 9, 0.1, EPS, 0, ptr(colstat), ptr(colstat), ptr(cross), ctypes.byref(info)) == BAD_ARG
    assert forward(env, handle, a, b, 0.0, over={"eps": 0.0})[0] == OK        # the ends of the ranges are inside


def test_a_callers_arena(env, handle):
    lib = env["lib"]
    a, b = inputs()
    base = forward(env, handle, a, b, 0.1)[1]
    tiny = torch.empty(64, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, _ = forward(env, handle, a, b, 0.1)
    assert rc == E_WORKSPACE and untouched(out)
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, info = forward(env, handle, a, b, 0.1)
    assert rc == OK and info.arena_bytes == need.value and all(torch.equal(out[k], base[k]) for k in base)
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, _ = backward(env, handle, a, b, 0.1, out["colstat"], out["cross"], g)
    assert rc == E_WORKSPACE and untouched(grads)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws2 = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws2.data_ptr(), ws2.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, info = backward(env, handle, a, b, 0.1, out["colstat"], out["cross"], g)
    assert rc == OK and info.arena_bytes == need.value and bool(torch.isfinite(grads["ga"]).all()) and not untouched(grads)
