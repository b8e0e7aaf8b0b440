"""rlap_edge_plan_build called through the C ABI on a handle of the test's own, after the pattern of tests/test_gpu_plan_cabi.py: the
arena the library owns, a caller's arena that is too small, one of exactly the size the library asks for; the plan moved into an
allocation of exactly plan_bytes; neither direction flag; and every refusal -- the host's and the device's -- with h_desc zeroed."""
import ctypes

import numpy as np
import pytest
import torch

import plan_buffer
from test_gpu_plan_cabi import BAD_ARG, E_WORKSPACE, OK, SPMM_CHUNK, TOO_LARGE, UNKNOWN_FLAG, desc_bytes, need_of, propagate, same_bits

pytestmark = pytest.mark.gpu

F = 4
INDEX_RANGE = 2


class Input:
    def __init__(self, ops, rows, ptr, n):
        self.sc, self.n = rows.contiguous(), n
        self.ptr = torch.as_tensor(ptr, dtype=torch.int64).to(rows.device)
        self.m, self.S = int(rows.shape[0]), self.ptr.numel() - 1
        self.x = (torch.arange(n * F, dtype=torch.float64, device=rows.device).reshape(n, F) % 17.0 - 8.0) / 4.0
        self.plan = ops.edge_list_plan(rows, ptr, n, weighted=True)
        self.decoded = plan_buffer.decode(self.plan.buffer.cpu().numpy(), self.plan.desc)
        self.y = [self.plan.propagate(self.x, transpose=t) for t in (False, True)]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib, graphs, ops
    rs = np.random.RandomState(1)
    n = 64
    ei = graphs.barabasi_albert(n, 3, 1).numpy()
    rows = np.stack([ei[0], ei[1], rs.rand(ei.shape[1]) + 0.5], 1).astype(np.float64)
    rows = np.concatenate([rows, [[5, 5, 2.0], [7, 7, 3.0], [5, 5, 4.0]]])     # directed, with loop rows; two segments in any order
    rs.shuffle(rows)
    small = Input(ops, torch.from_numpy(rows).cuda(), [0, 100, len(rows)], n)
    leaves = 2 * SPMM_CHUNK + 40
    w = rs.rand(leaves) + 0.5
    star = np.array([[i + 1, 0, w[i]] for i in range(leaves)] + [[0, i + 1, w[i]] for i in range(leaves)])
    rs.shuffle(star)
    stars = Input(ops, torch.from_numpy(star).cuda(), [0, len(star)], leaves + 1)
    assert small.plan.desc.chunks_forward == 0 and stars.plan.desc.chunks_forward == 3 and stars.plan.desc.chunks_transposed == 3
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
    return env["_lib"].GCN_WEIGHTED | env["_lib"].GCN_SELF_LOOPS | env["_lib"].GCN_NORMALIZE


def bound_of(env, inp, flags=None):
    b = ctypes.c_size_t(0)
    assert env["lib"].rlap_snapshot_plan_bytes(inp.m, inp.S, 1, inp.n, default_flags(env) if flags is None else flags, ctypes.byref(b)) == OK
    return int(b.value)


def build(env, h, inp, flags=None, buf=None, d_plan="buf", plan_bytes=None, sc=None, ptr=None, n=None):
    """One rlap_edge_plan_build on the handle; h_desc holds 0xFF bytes before the call.  Returns (status, desc, info, buf)."""
    lib, _lib = env["lib"], env["_lib"]
    if buf is None:
        buf = torch.empty(bound_of(env, inp), dtype=torch.uint8, device=inp.sc.device)
    desc, info = _lib.PlanDesc(), _lib.PlanInfo()
    ctypes.memset(ctypes.addressof(desc), 0xFF, ctypes.sizeof(desc))
    sc = inp.sc if sc is None else sc
    ptr = inp.ptr if ptr is None else ptr
    torch.cuda.synchronize()
    rc = lib.rlap_edge_plan_build(h, sc.data_ptr(), inp.m, ptr.data_ptr(), inp.S, None, 1, inp.n if n is None else n,
                                  default_flags(env) if flags is None else flags, 1.0, buf.data_ptr() if d_plan == "buf" else d_plan,
                                  buf.numel() if plan_bytes is None else plan_bytes, ctypes.byref(desc), ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, desc, info, buf


def check_products(env, h, inp, d_plan, desc):
    for t in (False, True):
        rc, info, y = propagate(env, h, d_plan, desc, inp.x, env["_lib"].SPMM_TRANSPOSE if t else 0, layers=inp.S)
        assert rc == OK and info.host_syncs == 0
        same_bits(y, inp.y[t])


def zeroed(desc):
    return desc_bytes(desc) == bytes(ctypes.sizeof(desc))


@pytest.mark.parametrize("which", ["small", "stars"])
def test_owned_arena_short_arena_exact_arena(env, handle, which):
    lib, inp = env["lib"], env[which]
    dev = inp.sc.device
    rc, desc, info, buf = build(env, handle, inp)
    assert rc == OK and desc.magic == env["_lib"].PLAN_MAGIC and info.host_syncs == 1 and info.entries == inp.plan.entries
    assert desc_bytes(desc) == desc_bytes(inp.plan.desc) and info.blocks == inp.plan.info["blocks"]
    first = plan_buffer.decode(buf.cpu().numpy(), desc)
    assert plan_buffer.same_decoded(first, inp.decoded)
    check_products(env, handle, inp, buf.data_ptr(), desc)
    short = torch.empty(256, dtype=torch.uint8, device=dev)                     # a caller's arena of 256 bytes: refused, h_desc zeroed
    assert lib.rlap_set_workspace(handle, short.data_ptr(), 256, None, 0) == 0
    rc, bad, _, _ = build(env, handle, inp)
    assert rc == E_WORKSPACE and zeroed(bad)
    need = need_of(env, handle)
    assert need > 256
    exact = torch.empty(need, dtype=torch.uint8, device=dev)                    # exactly the size the build asked for
    assert lib.rlap_set_workspace(handle, exact.data_ptr(), need, None, 0) == 0
    rc, desc2, info2, buf2 = build(env, handle, inp)
    assert rc == OK and info2.arena_bytes == need and desc_bytes(desc2) == desc_bytes(desc)
    assert plan_buffer.same_decoded(plan_buffer.decode(buf2.cpu().numpy(), desc2), first)


@pytest.mark.parametrize("which", ["small", "stars"])
def test_plan_moved_into_an_allocation_of_exactly_plan_bytes(env, handle, which):
    inp = env[which]
    rc, desc, _, buf = build(env, handle, inp)
    assert rc == OK
    used = int(desc.plan_bytes)
    assert 0 < used <= buf.numel()
    tight = torch.empty(used, dtype=torch.uint8, device=inp.sc.device)
    tight.copy_(buf[:used])
    buf.fill_(0xFF)                                                           # the build's buffer is gone
    check_products(env, handle, inp, tight.data_ptr(), desc)


def test_no_direction_flag_builds_both(env, handle):
    _lib, inp = env["_lib"], env["small"]
    both = _lib.PLAN_FORWARD | _lib.PLAN_TRANSPOSED
    rc, desc, info, buf = build(env, handle, inp, flags=default_flags(env))
    assert rc == OK and desc.flags == default_flags(env) | both
    assert desc.entries_forward == desc.entries_transposed == inp.m - 3 and info.loops_removed == 3
    assert plan_buffer.same_decoded(plan_buffer.decode(buf.cpu().numpy(), desc), inp.decoded)
    rc, one, info1, _ = build(env, handle, inp, flags=default_flags(env) | _lib.PLAN_TRANSPOSED)
    assert rc == OK and one.flags & both == _lib.PLAN_TRANSPOSED and one.entries_forward == -1 and info1.chunked_lists_forward == -1
    assert info1.blocks == info.blocks                                        # (the forward lists are counted by every build)


def test_every_refusal_zeroes_the_descriptor(env, handle):
    inp = env["small"]
    dev = inp.sc.device
    bound = bound_of(env, inp)
    buf = torch.full((bound + 16,), 0x5A, dtype=torch.uint8, device=dev)
    host = [("plan_bytes = bound - 1", dict(plan_bytes=bound - 1), BAD_ARG), ("d_plan + 8", dict(d_plan=buf.data_ptr() + 8, plan_bytes=bound), BAD_ARG),
            ("an unknown flag", dict(flags=default_flags(env) | UNKNOWN_FLAG, plan_bytes=bound), BAD_ARG),
            ("NULL d_plan", dict(d_plan=None, plan_bytes=bound), BAD_ARG), ("num_nodes = 2^31 - 1", dict(n=2 ** 31 - 1, plan_bytes=bound), TOO_LARGE)]
    for what, over, status in host:
        rc, desc, _, _ = build(env, handle, inp, buf=buf, **over)
        assert rc == status, (what, rc)
        assert zeroed(desc), f"{what}: h_desc is not zeroed"
        assert bool((buf == 0x5A).all()), f"{what}: the buffer was written"

    def altered(r, c, v):
        t = inp.sc.clone()
        t[r, c] = v
        return t
    bad_ptr = inp.ptr.clone()
    bad_ptr[1] = inp.m + 5                                                    # a ptr past m
    device = [("id 1.5", dict(sc=altered(3, 0, 1.5)), INDEX_RANGE), ("id -1", dict(sc=altered(4, 1, -1.0)), INDEX_RANGE),
              ("id num_nodes", dict(sc=altered(0, 1, float(inp.n))), INDEX_RANGE), ("NaN weight", dict(sc=altered(2, 2, float("nan"))), BAD_ARG),
              ("weight 0", dict(sc=altered(6, 2, 0.0)), BAD_ARG), ("a ptr past m", dict(ptr=bad_ptr), BAD_ARG),
              ("a decreasing ptr", dict(ptr=torch.tensor([0, 120, inp.m], device=dev).flip(0).contiguous()), BAD_ARG)]
    for what, over, status in device:
        rc, desc, info, _ = build(env, handle, inp, **over)
        assert rc == status, (what, rc)
        assert zeroed(desc) and info.host_syncs == 1, what
    rc, desc, _, _ = build(env, handle, inp, buf=buf, plan_bytes=bound)           # the handle is intact
    assert rc == OK
    check_products(env, handle, inp, buf.data_ptr(), desc)
