"""The two CCA exports (rlap_cca_loss / rlap_cca_loss_backward) called through the C ABI on raw device pointers and a handle of the
test's own, after the pattern of tests/test_gpu_infonce_cabi.py: one good call of each against ops.cca_loss; the statuses of the host
checks, which answer before anything is launched (the result buffers are filled with a pattern first and must come back
unchanged); a caller's arena that is too small and one of the size the library then asks for."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
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
    a = torch.randn(n, f, generator=g) + 0.5
    return a.cuda(), (0.3 * a + torch.randn(n, f, generator=g)).cuda()


def forward(env, h, a, b, lambd, flags=0, over=None):
    n, f = a.shape
    out = {"terms": torch.full((4,), PATTERN, dtype=torch.float64, device="cuda"),
           "colstat": torch.full((4 * f,), PATTERN, dtype=torch.float64, device="cuda"),
           "gram": torch.full((2, f, f), PATTERN, dtype=torch.float32, device="cuda")}
    info = env["_lib"].CcaInfo()
    c = {"a": ptr(a), "b": ptr(b), "N": n, "F": f, "lambd": lambd, "flags": flags, "terms": ptr(out["terms"]), "colstat": ptr(out["colstat"]),
         "gram": ptr(out["gram"])}
    c.update(over or {})
    rc = env["lib"].rlap_cca_loss(h, c["a"], c["b"], c["N"], c["F"], c["lambd"], c["flags"], c["terms"], c["colstat"], c["gram"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def backward(env, h, a, b, lambd, colstat, gram, g, flags=0, over=None):
    n, f = a.shape
    out = {k: torch.full((n, f), PATTERN, dtype=torch.float32, device="cuda") for k in ("ga", "gb")}
    info = env["_lib"].CcaInfo()
    c = {"a": ptr(a), "b": ptr(b), "N": n, "F": f, "lambd": lambd, "flags": flags, "colstat": ptr(colstat), "gram": ptr(gram), "g": ptr(g),
         "ga": ptr(out["ga"]), "gb": ptr(out["gb"])}
    c.update(over or {})
    rc = env["lib"].rlap_cca_loss_backward(h, c["a"], c["b"], c["N"], c["F"], c["lambd"], c["flags"], c["colstat"], c["gram"], c["g"], c["ga"],
                                           c["gb"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def untouched(out):
    return all(bool((t == PATTERN).all()) for t in out.values())


@pytest.mark.parametrize("lambd", [1e-3, 0.5])
def test_both_exports_on_raw_pointers(env, handle, lambd):
    from rlap_amd import ops
    a, b = inputs()
    rc, out, info = forward(env, handle, a, b, lambd)
    assert rc == OK and (info.rows, info.features, info.parts, info.host_syncs) == (70, 9, 3, 0) and info.arena_bytes > 0
    ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    terms = ops.cca_loss(ta, tb, lambd=lambd, return_terms=True)
    assert torch.equal(out["terms"], torch.stack([t.detach() for t in terms]))
    assert bool(torch.isfinite(out["colstat"]).all()) and torch.equal(out["gram"], out["gram"].transpose(1, 2))
    g = torch.tensor([1.5], dtype=torch.float64, device="cuda")
    rc, grads, info = backward(env, handle, a, b, lambd, out["colstat"], out["gram"], g)
    assert rc == OK and info.host_syncs == 0 and info.rows == 70
    (1.5 * terms[0]).backward()
    assert torch.equal(grads["ga"], ta.grad) and torch.equal(grads["gb"], tb.grad)


def test_host_checks_answer_before_anything_is_launched(env, handle):
    a, b = inputs()
    colstat = torch.ones(36, dtype=torch.float64, device="cuda")
    gram = torch.ones(2, 9, 9, dtype=torch.float32, device="cuda")
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    shared = [
        ({"lambd": -1e-3}, BAD_ARG), ({"lambd": float("nan")}, BAD_ARG), ({"lambd": float("inf")}, BAD_ARG),
        ({"F": 0}, BAD_ARG), ({"F": 513}, BAD_ARG), ({"N": 1}, BAD_ARG), ({"N": 0}, BAD_ARG), ({"N": -1}, BAD_ARG),
        ({"a": None}, BAD_ARG), ({"b": None}, BAD_ARG), ({"flags": 1}, BAD_ARG), ({"flags": 1 << 20}, BAD_ARG),
        ({"N": 1 << 31}, TOO_LARGE),
    ]
    for over, want in shared + [({"terms": None}, BAD_ARG), ({"colstat": None}, BAD_ARG), ({"gram": None}, BAD_ARG)]:
        rc, out, _ = forward(env, handle, a, b, 1e-3, over=over)
        assert rc == want and untouched(out), over
    for over, want in shared + [({"colstat": None}, BAD_ARG), ({"gram": None}, BAD_ARG), ({"g": None}, BAD_ARG), ({"ga": None}, BAD_ARG),
                                ({"gb": None}, BAD_ARG)]:
        rc, out, _ = backward(env, handle, a, b, 1e-3, colstat, gram, g, over=over)
        assert rc == want and untouched(out), over
    info = env["_lib"].CcaInfo()
    assert env["lib"].rlap_cca_loss(None, ptr(a), ptr(b), 70, 9, 1e-3, 0, ptr(colstat), ptr(colstat), ptr(gram), ctypes.byref(info)) == BAD_ARG
    assert forward(env, handle, a, b, 0.0)[0] == OK                   # the end of the range is inside


def test_a_callers_arena(env, handle):
    lib = env["lib"]
    a, b = inputs()
    base = forward(env, handle, a, b, 1e-3)[1]
    tiny = torch.empty(64, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, _ = forward(env, handle, a, b, 1e-3)
    assert rc == E_WORKSPACE and untouched(out)
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, info = forward(env, handle, a, b, 1e-3)
    assert rc == OK and info.arena_bytes == need.value and all(torch.equal(out[k], base[k]) for k in base)
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, _ = backward(env, handle, a, b, 1e-3, out["colstat"], out["gram"], g)
    assert rc == E_WORKSPACE and untouched(grads)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws2 = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws2.data_ptr(), ws2.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, info = backward(env, handle, a, b, 1e-3, out["colstat"], out["gram"], g)
    assert rc == OK and info.arena_bytes == need.value and bool(torch.isfinite(grads["ga"]).all()) and not untouched(grads)
