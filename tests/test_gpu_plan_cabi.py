"""The three plan exports (rlap_snapshot_plan_bytes / _plan_build / _plan_propagate) called through the C ABI on a handle of the
test's own, after the pattern of tests/test_gpu_snapshot_cabi.py: the arena the library owns, a caller's arena that is too small,
one of exactly the size the library asks for; the promises that only a C caller can exercise -- the buffer is the caller's and can
be moved, only desc.plan_bytes bytes of it are in use, d_x and d_y need no more than their type's alignment -- and the statuses of
the host checks, which answer before anything is launched (y is filled with a pattern first and must come back unchanged).

No case hands the device a buffer or a descriptor that the host accepts and that differs from what a build wrote."""
import ctypes

import pytest
import torch

import plan_buffer
from test_gpu_plan import two_stars

pytestmark = pytest.mark.gpu

N = 64                 # num_nodes of the small input
S = 2                  # two views
F = 4                  # feature columns
OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
UNKNOWN_FLAG = 1 << 20
INT32_MAX = 2 ** 31 - 1
SPMM_CHUNK = 256       # (rlap_spmm.h's CHUNK, documented in include/rlap_hip.h)


class Input:
    def __init__(self, ops, sc, ptr, n):
        self.sc, self.n = sc.contiguous(), n
        self.ptr = torch.as_tensor(ptr, dtype=torch.int64).to(sc.device)
        self.m, self.S = int(sc.shape[0]), self.ptr.numel() - 1
        self.x = (torch.arange(n * F, dtype=torch.float64, device=sc.device).reshape(n, F) % 17.0 - 8.0) / 4.0
        self.plan = ops.snapshot_plan(sc, ptr, n)
        self.decoded = plan_buffer.decode(self.plan.buffer.cpu().numpy(), self.plan.desc)
        self.y = [self.plan.propagate(self.x, transpose=t) for t in (False, True)]
        self.y32 = [self.plan.propagate(self.x.float(), transpose=t) for t in (False, True)]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib, graphs, ops
    sc, ptr = ops.approximate_cholesky_views(graphs.barabasi_albert(N, 3, 1), None, N, [16, 16], "degree", "asc")
    assert ptr.numel() == S + 1 and sc.is_cuda
    small = Input(ops, sc, ptr, N)
    stars = Input(ops, *two_stars(2 * SPMM_CHUNK + 40))
    assert small.plan.desc.chunks_forward == 0 and stars.plan.desc.chunks_forward == 6 and stars.plan.desc.chunks_transposed == 6
    torch.cuda.synchronize()
    return {"lib": _lib.load(), "_lib": _lib, "small": small, "stars": stars}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def default_flags(env):
    return env["_lib"].GCN_SELF_LOOPS | env["_lib"].GCN_NORMALIZE


def bound_of(env, inp, flags=None):
    b = ctypes.c_size_t(0)
    assert env["lib"].rlap_snapshot_plan_bytes(inp.m, inp.S, 1, inp.n, default_flags(env) if flags is None else flags, ctypes.byref(b)) == OK
    return int(b.value)


def desc_bytes(desc):
    return bytes(ctypes.string_at(ctypes.addressof(desc), ctypes.sizeof(desc)))


def build(env, h, inp, flags=None, buf=None, d_plan="buf", plan_bytes=None):
    """One rlap_snapshot_plan_build on the handle; h_desc holds 0xFF bytes before the call.  Returns (status, desc, info, buf)."""
    lib, _lib = env["lib"], env["_lib"]
    if buf is None:
        buf = torch.empty(bound_of(env, inp), dtype=torch.uint8, device=inp.sc.device)
    desc, info = _lib.PlanDesc(), _lib.PlanInfo()
    ctypes.memset(ctypes.addressof(desc), 0xFF, ctypes.sizeof(desc))
    torch.cuda.synchronize()
    rc = lib.rlap_snapshot_plan_build(h, inp.sc.data_ptr(), inp.m, inp.ptr.data_ptr(), inp.S, None, 1, inp.n,
                                      default_flags(env) if flags is None else flags, 1.0, buf.data_ptr() if d_plan == "buf" else d_plan,
                                      buf.numel() if plan_bytes is None else plan_bytes, ctypes.byref(desc), ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, desc, info, buf


def propagate(env, h, d_plan, desc, x, flags=0, Fcols=F, y=None, layers=None):
    """One rlap_snapshot_plan_propagate; returns (status, info, y)."""
    lib, _lib = env["lib"], env["_lib"]
    if y is None:
        y = torch.full((layers, x.shape[-2], x.shape[-1]), float("nan"), dtype=x.dtype, device=x.device)
    if x.dtype == torch.float32:
        flags |= _lib.SPMM_X_F32
    info = _lib.SpmmInfo()
    torch.cuda.synchronize()
    rc = lib.rlap_snapshot_plan_propagate(h, d_plan, ctypes.byref(desc), flags, x.data_ptr(), Fcols, y.data_ptr(), ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, info, y


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, tuple(got.shape), tuple(want.shape))
    view = torch.int64 if got.dtype == torch.float64 else torch.int32
    assert torch.equal(got.contiguous().view(view), want.contiguous().view(view))


def check_products(env, h, inp, d_plan, desc):
    for t in (False, True):
        rc, info, y = propagate(env, h, d_plan, desc, inp.x, env["_lib"].SPMM_TRANSPOSE if t else 0, layers=inp.S)
        assert rc == OK and info.host_syncs == 0
        same_bits(y, inp.y[t])


def need_of(env, h):
    need, rng = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert env["lib"].rlap_workspace_needed(h, ctypes.byref(need), ctypes.byref(rng)) == 0
    return int(need.value)


# ------------------------------------------------------------------------------------------------ 1. arenas
@pytest.mark.parametrize("which", ["small", "stars"])
def test_owned_arena_short_arena_exact_arena(env, handle, which):
    lib, inp = env["lib"], env[which]
    dev = inp.sc.device
    # the library's own arena: the buffer and the products of ops
    rc, desc, info, buf = build(env, handle, inp)
    assert rc == OK and desc.magic == env["_lib"].PLAN_MAGIC and info.host_syncs == 1 and info.entries == inp.plan.entries
    assert desc_bytes(desc) == desc_bytes(inp.plan.desc)
    first = plan_buffer.decode(buf.cpu().numpy(), desc)
    assert plan_buffer.same_decoded(first, inp.decoded)
    check_products(env, handle, inp, buf.data_ptr(), desc)
    # a caller's arena of 256 bytes: the build is refused, h_desc zeroed, the size it takes reported
    short = torch.empty(256, dtype=torch.uint8, device=dev)
    assert lib.rlap_set_workspace(handle, short.data_ptr(), 256, None, 0) == 0
    rc, bad, _, _ = build(env, handle, inp)
    assert rc == E_WORKSPACE and desc_bytes(bad) == bytes(ctypes.sizeof(bad))
    need = need_of(env, handle)
    assert need > 256
    # the planned call on that arena: without long lists it needs no more
    for t in (False, True):
        rc, pinfo, y = propagate(env, handle, buf.data_ptr(), desc, inp.x, env["_lib"].SPMM_TRANSPOSE if t else 0, layers=inp.S)
        if which == "small":
            assert rc == OK and pinfo.arena_bytes == 256 == need_of(env, handle)
            same_bits(y, inp.y[t])
        else:
            assert rc == E_WORKSPACE and need_of(env, handle) > 256
    # exactly the size the build asked for
    exact = torch.empty(need, dtype=torch.uint8, device=dev)
    assert lib.rlap_set_workspace(handle, exact.data_ptr(), need, None, 0) == 0
    rc, desc2, info2, buf2 = build(env, handle, inp)
    assert rc == OK and info2.arena_bytes == need and desc_bytes(desc2) == desc_bytes(desc)
    assert plan_buffer.same_decoded(plan_buffer.decode(buf2.cpu().numpy(), desc2), first)
    if which == "stars":   # exactly the size the planned call asked for
        for t in (False, True):
            flags = env["_lib"].SPMM_TRANSPOSE if t else 0
            assert lib.rlap_set_workspace(handle, short.data_ptr(), 256, None, 0) == 0
            assert propagate(env, handle, buf2.data_ptr(), desc2, inp.x, flags, layers=inp.S)[0] == E_WORKSPACE
            pneed = need_of(env, handle)
            assert pneed == 8 * 6 * F + 256                                   # six chunk sums of F doubles
            arena = torch.empty(pneed, dtype=torch.uint8, device=dev)
            assert lib.rlap_set_workspace(handle, arena.data_ptr(), pneed, None, 0) == 0
            rc, pinfo, y = propagate(env, handle, buf2.data_ptr(), desc2, inp.x, flags, layers=inp.S)
            assert rc == OK and pinfo.arena_bytes == pneed
            same_bits(y, inp.y[t])


def test_no_direction_flag_builds_both(env, handle):
    _lib, inp = env["_lib"], env["small"]
    both = _lib.PLAN_FORWARD | _lib.PLAN_TRANSPOSED
    assert bound_of(env, inp) == bound_of(env, inp, default_flags(env) | both)
    rc, desc, info, buf = build(env, handle, inp, flags=default_flags(env))
    assert rc == OK and desc.flags & both == both and desc.flags == default_flags(env) | both
    assert desc.entries_forward == desc.entries_transposed == inp.m and info.chunked_lists_forward == 0 and info.chunked_lists_transposed == 0
    rc, one, info1, _ = build(env, handle, inp, flags=default_flags(env) | _lib.PLAN_FORWARD)
    assert rc == OK and one.flags & both == _lib.PLAN_FORWARD and one.entries_transposed == -1 and info1.chunked_lists_transposed == -1
    assert bound_of(env, inp, default_flags(env) | _lib.PLAN_FORWARD) < bound_of(env, inp)


# ------------------------------------------------------------------------------------------------ 2. the buffer is the caller's
@pytest.mark.parametrize("which", ["small", "stars"])
def test_moved_buffers(env, handle, which):
    inp = env[which]
    dev = inp.sc.device
    rc, desc, _, buf = build(env, handle, inp)
    assert rc == OK
    used = int(desc.plan_bytes)
    assert 0 < used <= buf.numel()
    tight = torch.empty(used, dtype=torch.uint8, device=dev)                    # exactly the bytes in use
    tight.copy_(buf[:used])
    big = torch.full((used + 512,), 0xA5, dtype=torch.uint8, device=dev)        # a larger allocation, the plan 16 bytes into it
    big[16:16 + used].copy_(buf[:used])
    d_moved = big.data_ptr() + 16
    assert d_moved % 16 == 0 and d_moved % 256 != 0
    buf.fill_(0xFF)                                                           # the build's buffer is gone
    check_products(env, handle, inp, tight.data_ptr(), desc)
    check_products(env, handle, inp, d_moved, desc)
    assert bool((big[:16] == 0xA5).all()) and bool((big[16 + used:] == 0xA5).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("which", ["small", "stars"])
def test_misaligned_x_and_misaligned_y(env, handle, which, dtype):
    """F = 4 would take the 16-byte-a-lane kernels; a d_x or a d_y one element past a 16-byte boundary must take the one-column
    kernels: the bits of the aligned call."""
    _lib, inp = env["_lib"], env[which]
    dev = inp.sc.device
    rc, desc, _, buf = build(env, handle, inp)
    assert rc == OK
    x = inp.x.to(dtype)
    want = inp.y if dtype == torch.float64 else inp.y32
    count = inp.S * inp.n * F
    for t in (False, True):
        flags = _lib.SPMM_TRANSPOSE if t else 0
        rc, _, y = propagate(env, handle, buf.data_ptr(), desc, x, flags, layers=inp.S)
        assert rc == OK and x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
        same_bits(y, want[t])
        ybig = torch.full((count + 8,), -7.0, dtype=dtype, device=dev)        # y one element into a larger buffer
        yv = ybig[1:1 + count].view(inp.S, inp.n, F)
        assert yv.data_ptr() % 16 != 0 and yv.data_ptr() % yv.element_size() == 0
        rc, _, _ = propagate(env, handle, buf.data_ptr(), desc, x, flags, y=yv)
        assert rc == OK
        same_bits(yv, want[t])
        assert float(ybig[0]) == -7.0 and bool((ybig[1 + count:] == -7.0).all())   # nothing written beside y
        xbig = torch.zeros(inp.n * F + 8, dtype=dtype, device=dev)
        xbig[1:1 + inp.n * F] = x.reshape(-1)
        xv = xbig[1:1 + inp.n * F].view(inp.n, F)
        assert xv.data_ptr() % 16 != 0
        rc, _, y = propagate(env, handle, buf.data_ptr(), desc, xv, flags, layers=inp.S)
        assert rc == OK
        same_bits(y, want[t])


# ------------------------------------------------------------------------------------------------ 3. statuses of the host checks
def test_statuses_of_the_build(env, handle):
    """Honest calls that the host refuses: h_desc comes back all zero, nothing is launched."""
    inp = env["small"]
    bound = bound_of(env, inp)
    buf = torch.full((bound + 16,), 0x5A, dtype=torch.uint8, device=inp.sc.device)
    cases = [("plan_bytes = bound - 1", dict(plan_bytes=bound - 1)),
             ("d_plan + 8", dict(d_plan=buf.data_ptr() + 8, plan_bytes=bound)),
             ("an unknown flag", dict(flags=default_flags(env) | UNKNOWN_FLAG, plan_bytes=bound)),
             ("NULL d_plan", dict(d_plan=None, plan_bytes=bound))]
    for what, over in cases:
        rc, desc, _, _ = build(env, handle, inp, buf=buf, **over)
        assert rc == BAD_ARG, (what, rc)
        assert desc_bytes(desc) == bytes(ctypes.sizeof(desc)), f"{what}: h_desc is not zeroed"
        assert bool((buf == 0x5A).all()), f"{what}: the buffer was written"
    rc, desc, _, _ = build(env, handle, inp, buf=buf, plan_bytes=bound)           # the handle is intact
    assert rc == OK
    check_products(env, handle, inp, buf.data_ptr(), desc)


def copy_of(desc, **over):
    out = type(desc)()
    ctypes.memmove(ctypes.addressof(out), ctypes.addressof(desc), ctypes.sizeof(desc))
    for k, v in over.items():
        setattr(out, k, v)
    return out


def test_statuses_of_the_planned_call(env, handle):
    """Every descriptor below is refused by the host's checks of it; y holds a pattern and is unchanged after a synchronise."""
    _lib, inp = env["_lib"], env["small"]
    dev = inp.sc.device
    rc, desc, _, buf = build(env, handle, inp)
    assert rc == OK and desc.entries_forward == inp.m > 0
    rc, fwd, _, fbuf = build(env, handle, inp, flags=default_flags(env) | _lib.PLAN_FORWARD)
    assert rc == OK
    rc, tr, _, tbuf = build(env, handle, inp, flags=default_flags(env) | _lib.PLAN_TRANSPOSED)
    assert rc == OK
    T = _lib.SPMM_TRANSPOSE
    d_plan = buf.data_ptr()
    cases = [("magic cleared", d_plan, copy_of(desc, magic=0), 0, F),
             ("TRANSPOSE on a forward-only plan", fbuf.data_ptr(), fwd, T, F),
             ("forward on a transposed-only plan", tbuf.data_ptr(), tr, 0, F),
             ("F = 0", d_plan, desc, 0, 0),
             ("rec_forward = plan_bytes", d_plan, copy_of(desc, rec_forward=desc.plan_bytes), 0, F),
             ("entries_forward = m + 1", d_plan, copy_of(desc, entries_forward=inp.m + 1), 0, F),
             ("off_forward | 8", d_plan, copy_of(desc, off_forward=desc.off_forward | 8), 0, F),
             ("plan_bytes below the records' end", d_plan, copy_of(desc, plan_bytes=desc.rec_forward + 16 * desc.entries_forward - 16), 0, F),
             ("loop_offset = -1 with self loops", d_plan, copy_of(desc, loop_offset=-1), 0, F),
             ("d_plan + 8", d_plan + 8, desc, 0, F),
             ("an unknown flag", d_plan, desc, UNKNOWN_FLAG, F)]
    pattern = torch.full((inp.S, inp.n, F), -3.25, dtype=torch.float64, device=dev)
    for what, plan_ptr, d, flags, cols in cases:
        y = pattern.clone()
        rc, info, _ = propagate(env, handle, plan_ptr, d, inp.x, flags, Fcols=cols, y=y)
        assert rc == BAD_ARG, (what, rc)
        assert torch.equal(y, pattern), f"{what}: y was written"
        assert info.arena_bytes == 0 and info.entries == 0, what
    check_products(env, handle, inp, d_plan, desc)                               # the handle and the plan are intact
    for t, (p, d) in enumerate(((fbuf, fwd), (tbuf, tr))):
        rc, _, y = propagate(env, handle, p.data_ptr(), d, inp.x, T if t else 0, layers=inp.S)
        assert rc == OK
        same_bits(y, inp.y[t])


def test_statuses_of_the_size_query(env):
    lib, inp = env["lib"], env["small"]
    flags = default_flags(env)
    cases = [("S = 0", (inp.m, 0, 1, N, flags), BAD_ARG),
             ("G does not divide S", (inp.m, 2, 3, N, flags), BAD_ARG),
             ("an unknown flag", (inp.m, 2, 1, N, flags | UNKNOWN_FLAG), BAD_ARG),
             ("an unknown flag and num_nodes = INT32_MAX", (inp.m, 2, 1, INT32_MAX, flags | UNKNOWN_FLAG), BAD_ARG),
             ("num_nodes = INT32_MAX", (inp.m, 2, 1, INT32_MAX, flags), TOO_LARGE)]
    for what, args, status in cases:
        b = ctypes.c_size_t(0)
        assert lib.rlap_snapshot_plan_bytes(*args, ctypes.byref(b)) == status, what
    assert lib.rlap_snapshot_plan_bytes(inp.m, 2, 1, N, flags, None) == BAD_ARG
    assert bound_of(env, inp) >= 2 * 16 * inp.m + 8 * S * N + 2 * 8 * (S * N + 1)
