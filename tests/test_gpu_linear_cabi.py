"""The two dense-layer exports (rlap_linear_act / rlap_linear_act_backward) called through the C ABI on raw device pointers and a
handle of the test's own, after the pattern of tests/test_gpu_bt_cabi.py: good calls against ops.linear_act with every result inside
a larger buffer filled with a pattern, whose margins -- the rows behind M and whatever lies in front -- must come back unchanged;
each gradient absent in turn, no bias, the (Fout, Fin) layout; the statuses of the host checks, which answer before anything is
launched; a caller's arena one byte short of what the call needs; the parts and the arena bytes the header predicts."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
PATTERN = -7.25
MARGIN = 97          # floats in front of and behind every result (odd: the results start off the 16-byte grid)
NONE, RELU, ELU = 0, 1, 2
OUT_IN = 1


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


class Framed:
    """A result of `count` floats inside a buffer with MARGIN floats of the pattern on either side."""

    def __init__(self, *shape):
        self.shape = shape
        count = 1
        for s in shape:
            count *= s
        self.buf = torch.full((count + 2 * MARGIN,), PATTERN, dtype=torch.float32, device="cuda")
        self.body = self.buf[MARGIN:MARGIN + count]

    def ptr(self):
        return ctypes.c_void_p(self.body.data_ptr())

    def value(self):
        return self.body.view(*self.shape)

    def margins_intact(self):
        return bool((self.buf[:MARGIN] == PATTERN).all()) and bool((self.buf[-MARGIN:] == PATTERN).all())

    def untouched(self):
        return bool((self.buf == PATTERN).all())


def inputs(m=70, fin=9, fout=13, seed=1):
    g = torch.Generator().manual_seed(seed + m + fin + fout)
    x = torch.randn(m, fin, generator=g) + 0.25
    w = torch.randn(fin, fout, generator=g) / fin ** 0.5
    b = 0.5 * torch.randn(fout, generator=g)
    gy = torch.randn(m, fout, generator=g)
    return x.cuda(), w.cuda(), b.cuda(), gy.cuda()


def forward(env, h, x, w, b, act=NONE, alpha=1.0, flags=0, over=None):
    m, fin = x.shape
    fout = w.shape[0] if flags & OUT_IN else w.shape[1]
    y = Framed(m, fout)
    info = env["_lib"].LinearInfo()
    c = {"x": ptr(x), "M": m, "Fin": fin, "Fout": fout, "w": ptr(w), "b": ptr(b), "act": act, "alpha": alpha, "flags": flags, "y": y.ptr()}
    c.update(over or {})
    rc = env["lib"].rlap_linear_act(h, c["x"], c["M"], c["Fin"], c["Fout"], c["w"], c["b"], c["act"], c["alpha"], c["flags"], c["y"],
                                    ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, y, info


def backward(env, h, x, w, y, gy, act=NONE, alpha=1.0, flags=0, want=("gx", "gw", "gb"), over=None):
    m, fin = x.shape
    fout = gy.shape[1]
    out = {"gx": Framed(m, fin), "gw": Framed(*w.shape), "gb": Framed(fout)}
    info = env["_lib"].LinearInfo()
    c = {"x": ptr(x), "w": ptr(w), "y": ptr(y), "gy": ptr(gy), "M": m, "Fin": fin, "Fout": fout, "act": act, "alpha": alpha, "flags": flags}
    c.update({k: out[k].ptr() if k in want else None for k in out})
    c.update(over or {})
    rc = env["lib"].rlap_linear_act_backward(h, c["x"], c["w"], c["y"], c["gy"], c["M"], c["Fin"], c["Fout"], c["act"], c["alpha"], c["flags"],
                                             c["gx"], c["gw"], c["gb"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def aligned(n):
    return (n + 255) // 256 * 256


def pad32(f):
    return (f + 31) // 32 * 32


def predicted_bytes(m, fin, fout, backward=False, gx=True, gw=True, gb=True, parts=1):
    """rlap_linear.hip's carve: 256-byte aligned pieces and 256 bytes behind them."""
    off = 0
    if not backward or gx:
        off = aligned(off) + pad32(fin) * pad32(fout) * 4
    if backward and gw:
        off = aligned(off) + parts * pad32(fin) * pad32(fout) * 4
    if backward and gb:
        off = aligned(off) + ((m + 255) // 256) * fout * 8
    return off + 256


@pytest.mark.parametrize("m,fin,fout,act,flags", [(70, 9, 13, RELU, 0), (33, 32, 65, ELU, OUT_IN), (129, 65, 4, NONE, 0), (1, 1, 1, RELU, OUT_IN)])
def test_both_exports_on_raw_pointers_write_nothing_outside_their_results(env, handle, m, fin, fout, act, flags):
    from rlap_amd import ops
    x, w, b, gy = inputs(m, fin, fout)
    wl = w.t().contiguous() if flags else w
    parts = min((m + 31) // 32, 1024)                                          # one group of pairs at these widths: a part per row tile
    rc, y, info = forward(env, handle, x, wl, b, act, 0.75, flags)
    assert rc == OK and (info.rows, info.fin, info.fout, info.parts, info.host_syncs) == (m, fin, fout, parts, 0)
    assert info.arena_bytes == predicted_bytes(m, fin, fout)
    assert y.margins_intact()
    tx, tw, tb = (t.clone().requires_grad_(True) for t in (x, wl, b))
    name = {NONE: "none", RELU: "relu", ELU: "elu"}[act]
    want = ops.linear_act(tx, tw, tb, act=name, alpha=0.75, weight_layout="out_in" if flags else "in_out")
    assert torch.equal(y.value(), want)
    rc, out, info = backward(env, handle, x, wl, y.value(), gy, act, 0.75, flags)
    assert rc == OK and info.host_syncs == 0 and info.parts == parts
    assert info.arena_bytes == predicted_bytes(m, fin, fout, True, parts=parts)
    want.backward(gy)
    assert torch.equal(out["gx"].value(), tx.grad) and torch.equal(out["gw"].value(), tw.grad) and torch.equal(out["gb"].value(), tb.grad)
    assert all(o.margins_intact() for o in out.values())


@pytest.mark.parametrize("absent", ["gx", "gw", "gb"])
def test_an_absent_gradient_skips_its_kernels(env, handle, absent):
    x, w, b, gy = inputs()
    _, y, _ = forward(env, handle, x, w, b, ELU)
    _, full, _ = backward(env, handle, x, w, y.value(), gy, ELU)
    want = tuple(k for k in ("gx", "gw", "gb") if k != absent)
    rc, out, info = backward(env, handle, x, w, y.value(), gy, ELU, want=want)
    assert rc == OK and out[absent].untouched()
    assert all(torch.equal(out[k].value(), full[k].value()) and out[k].margins_intact() for k in want)
    assert info.arena_bytes == predicted_bytes(70, 9, 13, True, gx=absent != "gx", gw=absent != "gw", gb=absent != "gb", parts=3)
    assert info.arena_bytes < predicted_bytes(70, 9, 13, True, parts=3)


def test_no_bias_and_no_gradient_at_all(env, handle):
    x, w, b, gy = inputs()
    rc, y0, _ = forward(env, handle, x, w, None, NONE)
    rc1, y1, _ = forward(env, handle, x, w, torch.zeros_like(b), NONE)
    assert rc == OK and rc1 == OK and torch.equal(y0.value(), y1.value())       # v + 0 is v
    rc, out, info = backward(env, handle, x, w, y0.value(), gy, NONE, want=())
    assert rc == OK and all(o.untouched() for o in out.values()) and info.arena_bytes == 256


def test_host_checks_answer_before_anything_is_launched(env, handle):
    x, w, b, gy = inputs()
    y_in = torch.ones(70, 13, device="cuda")
    shared = [
        ({"alpha": 0.0}, BAD_ARG), ({"alpha": -1.0}, BAD_ARG), ({"alpha": float("nan")}, BAD_ARG), ({"alpha": float("inf")}, BAD_ARG),
        ({"act": 3}, BAD_ARG), ({"act": -1}, BAD_ARG), ({"flags": 2}, BAD_ARG), ({"flags": 3}, BAD_ARG), ({"flags": 1 << 20}, BAD_ARG),
        ({"Fin": 0}, BAD_ARG), ({"Fin": 513}, BAD_ARG), ({"Fout": 0}, BAD_ARG), ({"Fout": 513}, BAD_ARG), ({"M": 0}, BAD_ARG), ({"M": -1}, BAD_ARG),
        ({"x": None}, BAD_ARG), ({"w": None}, BAD_ARG), ({"M": 1 << 31}, TOO_LARGE),
    ]
    for over, want in shared + [({"y": None}, BAD_ARG)]:
        rc, y, info = forward(env, handle, x, w, b, RELU, over=over)
        assert rc == want and y.untouched() and info.arena_bytes == 0, over
    for over, want in shared + [({"y": None}, BAD_ARG), ({"gy": None}, BAD_ARG)]:
        rc, out, info = backward(env, handle, x, w, y_in, gy, RELU, over=over)
        assert rc == want and all(o.untouched() for o in out.values()) and info.arena_bytes == 0, over
    info = env["_lib"].LinearInfo()
    y = Framed(70, 13)
    assert env["lib"].rlap_linear_act(None, ptr(x), 70, 9, 13, ptr(w), ptr(b), 0, 1.0, 0, y.ptr(), ctypes.byref(info)) == BAD_ARG
    assert forward(env, handle, x, w, b, ELU, alpha=1e-300)[0] == OK             # the ends of the ranges are inside


def test_an_arena_one_byte_short(env, handle):
    lib = env["lib"]
    x, w, b, gy = inputs()
    _, base, _ = forward(env, handle, x, w, b, RELU)
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    need = predicted_bytes(70, 9, 13)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), need - 1, rng.data_ptr(), rng.numel()) == OK
    rc, y, _ = forward(env, handle, x, w, b, RELU)
    assert rc == E_WORKSPACE and y.untouched()
    asked, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(asked), ctypes.byref(rn)) == OK and asked.value == need
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), need, rng.data_ptr(), rng.numel()) == OK
    rc, y, info = forward(env, handle, x, w, b, RELU)
    assert rc == OK and info.arena_bytes == need and torch.equal(y.value(), base.value())
    need_b = predicted_bytes(70, 9, 13, True, parts=3)
    ws2 = torch.empty(need_b, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws2.data_ptr(), need_b - 1, rng.data_ptr(), rng.numel()) == OK
    rc, out, _ = backward(env, handle, x, w, y.value(), gy, RELU)
    assert rc == E_WORKSPACE and all(o.untouched() for o in out.values())
    assert lib.rlap_workspace_needed(handle, ctypes.byref(asked), ctypes.byref(rn)) == OK and asked.value == need_b
    assert lib.rlap_set_workspace(handle, ws2.data_ptr(), need_b, rng.data_ptr(), rng.numel()) == OK
    rc, out, info = backward(env, handle, x, w, y.value(), gy, RELU)
    assert rc == OK and info.arena_bytes == need_b and not out["gx"].untouched() and all(o.margins_intact() for o in out.values())


def test_a_poisoned_arena_changes_no_bit(env, handle):
    lib = env["lib"]
    x, w, b, gy = inputs(129, 33, 65)
    _, y, _ = forward(env, handle, x, w, b, ELU)
    _, out, _ = backward(env, handle, x, w, y.value(), gy, ELU)
    assert lib.rlap_debug_set_poison(handle, 0xFF) == OK
    _, y2, _ = forward(env, handle, x, w, b, ELU)
    _, out2, _ = backward(env, handle, x, w, y.value(), gy, ELU)
    assert lib.rlap_debug_set_poison(handle, -1) == OK
    assert torch.equal(y.value(), y2.value()) and all(torch.equal(out[k].value(), out2[k].value()) for k in out)
