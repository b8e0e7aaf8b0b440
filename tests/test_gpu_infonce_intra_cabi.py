"""The four exports with intraview negatives (rlap_infonce_intra, rlap_infonce_intra_backward, rlap_infonce_pair_intra,
rlap_infonce_pair_intra_backward) called through the C ABI on raw device pointers and a handle of the test's own, after the pattern of
tests/test_gpu_infonce_pair_cabi.py: one good call of each against ops; `intraview` of 0, 3 and -1 refused; the refusals of
rlap_infonce, which the new exports share and which answer before anything is launched (the result buffers are filled with a pattern
first and must come back unchanged); the plain exports still refusing flags = 2; a caller's arena that is too small and one of the
size the library then asks for, at N = 4096."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
RAW = 1
MASKED, ALL = 1, 2
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


def names(env, pair):
    stem = "rlap_infonce_pair_intra" if pair else "rlap_infonce_intra"
    return getattr(env["lib"], stem), getattr(env["lib"], stem + "_backward"), env["_lib"].InfoncePairInfo if pair else env["_lib"].InfonceInfo


def forward(env, h, pair, a, b, tau, flags, intraview, over=None):
    n, f = a.shape
    lists = 2 if pair else 1
    out = {k: torch.full((m,), PATTERN, dtype=torch.float64, device="cuda") for k, m in (("loss", 1), ("rows", lists * n), ("z", lists * n))}
    fn, _, info_cls = names(env, pair)
    info = info_cls()
    c = {"a": ptr(a), "b": ptr(b), "N": n, "F": f, "tau": tau, "flags": flags, "intraview": intraview, "loss": ptr(out["loss"]),
         "rows": ptr(out["rows"]), "z": ptr(out["z"])}
    c.update(over or {})
    rc = fn(h, c["a"], c["b"], c["N"], c["F"], c["tau"], c["flags"], c["intraview"], c["loss"], c["rows"], c["z"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def backward(env, h, pair, a, b, tau, flags, intraview, z, g, over=None):
    n, f = a.shape
    out = {k: torch.full((n, f), PATTERN, dtype=torch.float32, device="cuda") for k in ("ga", "gb")}
    _, fn, info_cls = names(env, pair)
    info = info_cls()
    c = {"a": ptr(a), "b": ptr(b), "N": n, "F": f, "tau": tau, "flags": flags, "intraview": intraview, "z": ptr(z), "g": ptr(g),
         "ga": ptr(out["ga"]), "gb": ptr(out["gb"])}
    c.update(over or {})
    rc = fn(h, c["a"], c["b"], c["N"], c["F"], c["tau"], c["flags"], c["intraview"], c["z"], c["g"], c["ga"], c["gb"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def untouched(out):
    return all(bool((t == PATTERN).all()) for t in out.values())


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("intraview,variant", [(MASKED, "masked"), (ALL, "all")])
@pytest.mark.parametrize("flags,positive", [(0, "scaled"), (RAW, "raw")])
def test_the_exports_on_raw_pointers(env, handle, pair, intraview, variant, flags, positive):
    from rlap_amd import ops
    a, b = inputs()
    rc, out, info = forward(env, handle, pair, a, b, 0.4, flags, intraview)
    assert rc == OK and (info.rows, info.features, info.parts, info.host_syncs) == (70, 9, 3, 0) and info.arena_bytes > 0
    if pair:
        assert info.groups == 1
    ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    loss, rows = (ops.info_nce_pair if pair else ops.info_nce)(ta, tb, tau=0.4, positive=positive, return_rows=True, intraview=variant)
    assert torch.equal(out["loss"][0], loss.detach()) and torch.equal(out["rows"].view(rows.shape), rows)
    g = torch.tensor([1.5], dtype=torch.float64, device="cuda")
    rc, grads, info = backward(env, handle, pair, a, b, 0.4, flags, intraview, out["z"], g)
    assert rc == OK and info.host_syncs == 0 and info.rows == 70
    (1.5 * loss).backward()
    assert torch.equal(grads["ga"], ta.grad) and torch.equal(grads["gb"], tb.grad)
    # the other variant gives other bits from the same pointers
    rc, other, _ = forward(env, handle, pair, a, b, 0.4, flags, MASKED + ALL - intraview)
    assert rc == OK and not torch.equal(other["z"], out["z"])


@pytest.mark.parametrize("pair", [False, True])
def test_host_checks_answer_before_anything_is_launched(env, handle, pair):
    a, b = inputs()
    z = torch.ones(140, dtype=torch.float64, device="cuda")
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    nan = float("nan")
    shared = [
        ({"intraview": 0}, BAD_ARG), ({"intraview": 3}, BAD_ARG), ({"intraview": -1}, BAD_ARG),
        ({"tau": 0.0}, BAD_ARG), ({"tau": 0.03}, BAD_ARG), ({"tau": 1024.5}, BAD_ARG), ({"tau": -0.4}, BAD_ARG), ({"tau": nan}, BAD_ARG),
        ({"F": 0}, BAD_ARG), ({"N": 0}, BAD_ARG), ({"N": -1}, BAD_ARG), ({"a": None}, BAD_ARG), ({"b": None}, BAD_ARG),
        ({"flags": 2}, BAD_ARG), ({"flags": 1 << 20}, BAD_ARG),
        ({"F": 513}, TOO_LARGE), ({"N": 1 << 31}, TOO_LARGE),
    ]
    for over, want in shared + [({"loss": None}, BAD_ARG), ({"rows": None}, BAD_ARG), ({"z": None}, BAD_ARG)]:
        rc, out, _ = forward(env, handle, pair, a, b, 0.4, 0, MASKED, over=over)
        assert rc == want and untouched(out), over
    for over, want in shared + [({"z": None}, BAD_ARG), ({"g": None}, BAD_ARG), ({"ga": None}, BAD_ARG), ({"gb": None}, BAD_ARG)]:
        rc, out, _ = backward(env, handle, pair, a, b, 0.4, 0, ALL, z, g, over=over)
        assert rc == want and untouched(out), over
    fn, _, info_cls = names(env, pair)
    info = info_cls()
    assert fn(None, ptr(a), ptr(b), 70, 9, 0.4, 0, MASKED, ptr(z), ptr(z), ptr(z), ctypes.byref(info)) == BAD_ARG
    for tau in (1.0 / 32.0, 1024.0):                                  # the ends of the range are inside
        assert forward(env, handle, pair, a, b, tau, 0, ALL)[0] == OK


def test_the_plain_exports_still_refuse_flags_2(env, handle):
    """`intraview` did not become a flag: the four exports without it take RLAP_INFONCE_POSITIVE_RAW alone."""
    lib, _lib = env["lib"], env["_lib"]
    a, b = inputs()
    out = torch.full((1 + 4 * 70,), PATTERN, dtype=torch.float64, device="cuda")
    grads = torch.full((2, 70, 9), PATTERN, dtype=torch.float32, device="cuda")
    z = torch.ones(140, dtype=torch.float64, device="cuda")
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    p = out.data_ptr()
    for fn, info in ((lib.rlap_infonce, _lib.InfonceInfo()), (lib.rlap_infonce_pair, _lib.InfoncePairInfo())):
        assert fn(handle, ptr(a), ptr(b), 70, 9, 0.4, 2, p, p + 8, p + 8 * 141, ctypes.byref(info)) == BAD_ARG
    for fn, info in ((lib.rlap_infonce_backward, _lib.InfonceInfo()), (lib.rlap_infonce_pair_backward, _lib.InfoncePairInfo())):
        assert fn(handle, ptr(a), ptr(b), 70, 9, 0.4, 2, ptr(z), ptr(g), ptr(grads[0]), ptr(grads[1]), ctypes.byref(info)) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((out == PATTERN).all()) and bool((grads == PATTERN).all())


@pytest.mark.parametrize("pair", [False, True])
def test_the_arena_query_equals_what_the_call_uses(env, handle, pair):
    """N = 4096 (eight parts): a caller's arena that is too small is refused with nothing written, the query then says how much, an
    arena of exactly that size serves, and the call reports that size; the forward call needs more than its plain counterpart (the
    intraview part sums), the backward call exactly as much."""
    lib = env["lib"]
    a, b = inputs(4096, 33)
    base = forward(env, handle, pair, a, b, 0.4, RAW, MASKED)[1]
    tiny = torch.empty(64, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)

    def needed():
        assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK
        return need.value
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, _ = forward(env, handle, pair, a, b, 0.4, RAW, MASKED)
    assert rc == E_WORKSPACE and untouched(out)
    fwd = needed()
    ws = torch.empty(fwd, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, info = forward(env, handle, pair, a, b, 0.4, RAW, MASKED)
    assert rc == OK and info.arena_bytes == fwd and all(torch.equal(out[k], base[k]) for k in base)
    g = torch.ones(1, dtype=torch.float64, device="cuda")
    rc, grads, _ = backward(env, handle, pair, a, b, 0.4, RAW, MASKED, out["z"], g)
    assert rc == E_WORKSPACE and untouched(grads)
    bwd = needed()
    assert bwd > fwd
    ws2 = torch.empty(bwd, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws2.data_ptr(), ws2.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, info = backward(env, handle, pair, a, b, 0.4, RAW, MASKED, out["z"], g)
    assert rc == OK and info.arena_bytes == bwd and bool(torch.isfinite(grads["ga"]).all()) and not untouched(grads)
    # the plain calls in the same arenas: the forward one fits with room to spare, the backward one needs exactly as much
    plain = lib.rlap_infonce_pair if pair else lib.rlap_infonce
    plain_back = lib.rlap_infonce_pair_backward if pair else lib.rlap_infonce_backward
    info = (env["_lib"].InfoncePairInfo if pair else env["_lib"].InfonceInfo)()
    lists = 2 if pair else 1
    o = torch.empty(1 + 2 * lists * 4096, dtype=torch.float64, device="cuda")
    p = o.data_ptr()
    assert plain(handle, ptr(a), ptr(b), 4096, 33, 0.4, RAW, p, p + 8, p + 8 * (1 + lists * 4096), ctypes.byref(info)) == OK
    npad, parts = 4096, 8
    assert fwd - info.arena_bytes == lists * parts * npad * 8                  # [parts, Np] doubles a view
    assert plain_back(handle, ptr(a), ptr(b), 4096, 33, 0.4, RAW, p + 8 * (1 + lists * 4096), ptr(g), ptr(grads["ga"]), ptr(grads["gb"]), ctypes.byref(info)) == OK
    torch.cuda.synchronize()
    assert info.arena_bytes == bwd
