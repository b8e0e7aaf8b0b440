"""The four graph-to-local exports (rlap_g2l_jsd / rlap_g2l_bootstrap and their backward calls) called through the C ABI on raw device
pointers and a handle of the test's own, after the pattern of tests/test_gpu_infonce_cabi.py: one good call of each against the ops;
the statuses of the host checks, one per refusal the header lists, which answer before anything is launched (the result buffers are
filled with a pattern first and must come back unchanged); a caller's arena that is too small and one of the size the library then
asks for."""
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


def inputs(n=70, G=3, f=9):
    gen = torch.Generator().manual_seed(n + G + f)
    h, neg = 0.5 * torch.randn(n, f, generator=gen), 0.5 * torch.randn(n, f, generator=gen)
    g = torch.randn(G, f, generator=gen)
    table = torch.tensor([(n * j) // G for j in range(G + 1)], dtype=torch.int64)
    return h.cuda(), (neg.cuda() if G == 1 else None), g.cuda(), table.cuda()


def call(env, h, name, x, neg, g, table, over=None, gup=None):
    """One export: (status, the result buffers, the info).  `over` replaces arguments by name."""
    n, f = x.shape
    G = g.shape[0]
    jsd, back = "jsd" in name, name.endswith("backward")
    f64 = lambda m: torch.full((m,), PATTERN, dtype=torch.float64, device="cuda")
    f32 = lambda *s: torch.full(s, PATTERN, dtype=torch.float32, device="cuda")
    if back:
        out = {"gh": f32(n, f)}
        if jsd:
            out["gg"] = f32(G, f)
            if neg is not None:
                out["gneg"] = f32(n, f)
    else:
        out = {"loss": f64(1), "rows": f64(2 * n if jsd else n)}
    c = {"x": ptr(x), "neg": ptr(neg), "g": ptr(g), "N": n, "F": f, "node_ptr": ptr(table), "G": G, "flags": 0, "gup": ptr(gup)}
    c.update({k: ptr(v) for k, v in out.items()})
    c.setdefault("gneg", None)
    c.update(over or {})
    info = env["_lib"].G2lInfo()
    lib = env["lib"]
    head = (h, c["x"]) + ((c["neg"],) if jsd else ()) + (c["g"], c["N"], c["F"], c["node_ptr"], c["G"], c["flags"])
    if back:
        tail = (c["gup"], c["gh"]) + ((c["gneg"], c["gg"]) if jsd else ())
    else:
        tail = (c["loss"], c["rows"])
    rc = getattr(lib, name)(*head, *tail, ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def untouched(out):
    return all(bool((t == PATTERN).all()) for t in out.values())


@pytest.mark.parametrize("G", [1, 3])
def test_the_four_exports_on_raw_pointers(env, handle, G):
    from rlap_amd import ops
    x, neg, g, table = inputs(G=G)
    rc, out, info = call(env, handle, "rlap_g2l_jsd", x, neg, g, table)
    assert rc == OK and (info.rows, info.graphs, info.features, info.host_syncs) == (70, G, 9, 0) and info.arena_bytes > 0 and info.parts >= 1
    tx, tg = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
    tn = neg.clone().requires_grad_(True) if neg is not None else None
    loss, rows = ops.g2l_jsd(tx, tg, node_ptr=table.cpu(), neg=tn, return_rows=True)
    assert torch.equal(out["loss"][0], loss.detach()) and torch.equal(out["rows"].view(2, 70), rows)
    gup = torch.tensor([1.5], dtype=torch.float64, device="cuda")
    rc, grads, info = call(env, handle, "rlap_g2l_jsd_backward", x, neg, g, table, gup=gup)
    assert rc == OK and info.host_syncs == 0 and info.rows == 70
    (1.5 * loss).backward()
    assert torch.equal(grads["gh"], tx.grad) and torch.equal(grads["gg"], tg.grad)
    if neg is not None:
        assert torch.equal(grads["gneg"], tn.grad)
    rc, out, info = call(env, handle, "rlap_g2l_bootstrap", x, None, g, table)
    assert rc == OK and (info.rows, info.graphs, info.features, info.host_syncs) == (70, G, 9, 0)
    tx = x.clone().requires_grad_(True)
    loss, rows = ops.g2l_bootstrap(tx, g, node_ptr=table.cpu(), return_rows=True)
    assert torch.equal(out["loss"][0], loss.detach()) and torch.equal(out["rows"], rows)
    rc, grads, info = call(env, handle, "rlap_g2l_bootstrap_backward", x, None, g, table, gup=gup)
    assert rc == OK and info.host_syncs == 0
    (1.5 * loss).backward()
    assert torch.equal(grads["gh"], tx.grad)


def test_host_checks_answer_before_anything_is_launched(env, handle):
    x, _, g, table = inputs(G=3)
    x1, neg1, g1, table1 = inputs(G=1)
    gup = torch.ones(1, dtype=torch.float64, device="cuda")
    shared = [
        ({"x": None}, BAD_ARG), ({"g": None}, BAD_ARG), ({"node_ptr": None}, BAD_ARG),
        ({"N": 0}, BAD_ARG), ({"N": -1}, BAD_ARG), ({"F": 0}, BAD_ARG), ({"G": 0}, BAD_ARG), ({"G": -2}, BAD_ARG),
        ({"flags": 1}, BAD_ARG), ({"flags": 1 << 20}, BAD_ARG),
        ({"F": 513}, TOO_LARGE), ({"N": 1 << 31}, TOO_LARGE), ({"G": 1 << 31}, TOO_LARGE),
    ]
    forward = [({"loss": None}, BAD_ARG), ({"rows": None}, BAD_ARG)]
    backward = [({"gup": None}, BAD_ARG), ({"gh": None}, BAD_ARG)]
    for name in ("rlap_g2l_jsd", "rlap_g2l_bootstrap"):
        for over, want in shared + forward:
            rc, out, info = call(env, handle, name, x, None, g, table, over=over)
            assert rc == want and untouched(out) and info.rows == 0, (name, over)
        for over, want in shared + backward + ([({"gg": None}, BAD_ARG)] if "jsd" in name else []):
            rc, out, info = call(env, handle, name + "_backward", x, None, g, table, over=over, gup=gup)
            assert rc == want and untouched(out), (name, over)
    # one graph without neg, several graphs with it; the gradient buffer of neg goes with neg
    for name in ("rlap_g2l_jsd", "rlap_g2l_jsd_backward"):
        rc, out, _ = call(env, handle, name, x1, None, g1, table1, gup=gup)
        assert rc == BAD_ARG and untouched(out), name
        rc, out, _ = call(env, handle, name, x, x, g, table, gup=gup)
        assert rc == BAD_ARG and untouched(out), name
    rc, out, _ = call(env, handle, "rlap_g2l_jsd_backward", x1, neg1, g1, table1, over={"gneg": None}, gup=gup)
    assert rc == BAD_ARG and untouched(out)
    info = env["_lib"].G2lInfo()
    assert env["lib"].rlap_g2l_bootstrap(None, ptr(x), ptr(g), 70, 9, ptr(table), 3, 0, ptr(gup), ptr(gup), ctypes.byref(info)) == BAD_ARG
    assert call(env, handle, "rlap_g2l_jsd", x1, neg1, g1, table1)[0] == OK


def test_a_table_that_is_not_well_formed_gives_numbers_not_a_fault(env, handle):
    """The table is the caller's to get right; the kernels clamp what they read from it before it becomes an address."""
    x, _, g, _ = inputs(G=3)
    bad = torch.tensor([-5, 1 << 40, 35, -(1 << 50)], dtype=torch.int64, device="cuda")
    for name in ("rlap_g2l_jsd", "rlap_g2l_bootstrap"):
        rc, out, _ = call(env, handle, name, x, None, g, bad)
        assert rc == OK and bool(torch.isfinite(out["loss"]).all()) and bool(torch.isfinite(out["rows"]).all())


def shifted(t):
    """The same values at an address that is 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("f", [9, 32])
def test_pointers_that_are_not_16_byte_aligned_give_the_same_bits(env, handle, f):
    """The vector kernels stage rows with 16-byte loads only where the address allows them; float32 buffers need 4-byte alignment
    and no more.  One graph (JSD with neg) and the bootstrap, forward and backward, aligned against shifted by one float."""
    x, neg, g, table = inputs(n=300, G=1, f=f)
    gup = torch.tensor([0.75], dtype=torch.float64, device="cuda")
    for name, nn in (("rlap_g2l_jsd", neg), ("rlap_g2l_jsd_backward", neg), ("rlap_g2l_bootstrap", None), ("rlap_g2l_bootstrap_backward", None)):
        rc, want, _ = call(env, handle, name, x, nn, g, table, gup=gup)
        assert rc == OK
        rc, got, _ = call(env, handle, name, shifted(x), shifted(nn) if nn is not None else None, shifted(g), table, gup=gup)
        assert rc == OK and all(torch.equal(got[k], want[k]) for k in want), name


def test_a_callers_arena(env, handle):
    lib = env["lib"]
    x, _, g, table = inputs(G=3)
    base = call(env, handle, "rlap_g2l_jsd", x, None, g, table)[1]
    tiny = torch.empty(64, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, _ = call(env, handle, "rlap_g2l_jsd", x, None, g, table)
    assert rc == E_WORKSPACE and untouched(out)
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, out, info = call(env, handle, "rlap_g2l_jsd", x, None, g, table)
    assert rc == OK and info.arena_bytes == need.value and all(torch.equal(out[k], base[k]) for k in base)
    gup = torch.ones(1, dtype=torch.float64, device="cuda")
    rc, grads, _ = call(env, handle, "rlap_g2l_jsd_backward", x, None, g, table, gup=gup)
    assert rc == E_WORKSPACE and untouched(grads)                      # the backward call needs more: both images of both inputs
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > ws.numel()
    ws2 = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws2.data_ptr(), ws2.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, grads, info = call(env, handle, "rlap_g2l_jsd_backward", x, None, g, table, gup=gup)
    assert rc == OK and info.arena_bytes == need.value and bool(torch.isfinite(grads["gh"]).all()) and not untouched(grads)
