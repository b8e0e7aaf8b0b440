"""The two readout exports (rlap_graph_readout / rlap_graph_readout_backward) called through the C ABI on raw device pointers and a
handle of the test's own, after the pattern of tests/test_gpu_plan_cabi.py: the arena the library owns, a caller's arena that is
too small and one of the size the library then asks for; the statuses of the host checks, which answer before anything is launched
(y is filled with a pattern first and must come back unchanged); what h_info reports without the table being read back; pointers off the 16-byte grid, which take the one-element kernels; and a
table that is not well formed on a tiny input -- decreasing, or ending beyond num_nodes -- which the kernels clamp: the call ends
cleanly with some numbers.  That case exercises the clamp; it provokes no error."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, BAD_ARG, TOO_LARGE, E_WORKSPACE = 0, 3, 9, 11
MEAN, X_F32 = 1, 32
UNKNOWN_FLAG = 1 << 20
SPMM_MAX_F = 65536      # (rlap_snapshot_propagate's limit, include/rlap_hip.h)
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
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def forward(env, h, x, node_ptr, flags, y=None, over=None):
    """One rlap_graph_readout on the handle: (status, y, info).  `over` replaces arguments of the C call by name."""
    L, N, F = x.shape
    G = node_ptr.numel() - 1
    if y is None:
        y = torch.full((L, G, F), PATTERN, dtype=x.dtype, device=x.device)
    info = env["_lib"].ReadoutInfo()
    a = {"x": ptr(x), "L": L, "N": N, "F": F, "node_ptr": ptr(node_ptr), "G": G, "flags": flags | (X_F32 if x.dtype == torch.float32 else 0), "y": ptr(y)}
    a.update(over or {})
    rc = env["lib"].rlap_graph_readout(h, a["x"], a["L"], a["N"], a["F"], a["node_ptr"], a["G"], a["flags"], a["y"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, y, info


def backward(env, h, gy, node_ptr, N, flags, over=None, gx=None):
    L, G, F = gy.shape
    if gx is None:
        gx = torch.full((L, N, F), PATTERN, dtype=gy.dtype, device=gy.device)
    info = env["_lib"].ReadoutInfo()
    a = {"gy": ptr(gy), "L": L, "N": N, "F": F, "node_ptr": ptr(node_ptr), "G": G, "flags": flags | (X_F32 if gy.dtype == torch.float32 else 0), "gx": ptr(gx)}
    a.update(over or {})
    rc = env["lib"].rlap_graph_readout_backward(h, a["gy"], a["L"], a["N"], a["F"], a["node_ptr"], a["G"], a["flags"], a["gx"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, gx, info


def small(dtype=torch.float64, N=700, F=6, L=2):
    x = ((torch.arange(L * N * F, dtype=torch.float64).reshape(L, N, F) % 23.0) - 11.0) / 8.0    # (exact in float32; sums exact in float64)
    node_ptr = torch.tensor([0, 300, 300, 301, N], dtype=torch.int64)
    return x.to(dtype).cuda(), node_ptr.cuda()


def exact(x, node_ptr, mean=False):
    """The readout of features whose sums are exact in float64, on the CPU (a true float64 division by the count for the mean: on
    the device torch divides by a scalar through its reciprocal, which rounds differently)."""
    p = node_ptr.cpu().tolist()
    xs = x.cpu().double()
    rows = torch.stack([xs[:, p[g]:p[g + 1]].sum(1) for g in range(len(p) - 1)], dim=1)
    if mean:
        rows = rows / torch.tensor([max(p[g + 1] - p[g], 1) for g in range(len(p) - 1)], dtype=torch.float64)[None, :, None]
    return rows.to(x.dtype).to(x.device)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_both_exports_on_raw_pointers(env, handle, dtype):
    x, node_ptr = small(dtype)
    for flags in (0, MEAN):
        rc, y, info = forward(env, handle, x, node_ptr, flags)
        assert rc == OK
        assert torch.equal(y, exact(x, node_ptr, flags == MEAN))     # (the sums of these features are exact: any order gives them)
        # h_info without reading the table back: the bounds for G > 1
        assert (info.rows, info.graphs, info.host_syncs) == (700, 4, 0) and info.arena_bytes > 0
        assert info.chunks == (700 + 255) // 256 + 4 and info.chunked_graphs == min(4, 700 // 257)
        gy = y
        rc, gx, info = backward(env, handle, gy, node_ptr, 700, flags)
        assert rc == OK and info.host_syncs == 0 and info.rows == 700
        p = node_ptr.cpu()
        batch = torch.repeat_interleave(torch.arange(4), p[1:] - p[:-1]).cuda()
        want = gy[:, batch]
        if flags == MEAN:
            want = (want.cpu().double() / (p[1:] - p[:-1]).double()[batch.cpu()][None, :, None]).to(dtype).cuda()
        assert torch.equal(gx, want)


def off_the_grid(t=None, shape=None, dtype=None):
    """(view, buffer): a contiguous view one element into a buffer filled with the pattern, holding t's values if given."""
    shape = tuple(t.shape) if t is not None else shape
    count = 1
    for s in shape:
        count *= s
    big = torch.full((count + 8,), PATTERN, dtype=t.dtype if t is not None else dtype, device="cuda")
    if t is not None:
        big[1:1 + count] = t.reshape(-1)
    v = big[1:1 + count].view(shape)
    assert big.data_ptr() % 16 == 0 and v.is_contiguous() and v.data_ptr() % 16 != 0 and v.data_ptr() % v.element_size() == 0
    return v, big


def bits_equal(a, b):
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


def around_intact(big, count):
    return float(big[0]) == PATTERN and bool((big[1 + count:] == PATTERN).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("F", [16, 200])
def test_misaligned_pointers(env, handle, F, dtype):
    """F = 16 and F = 200 take the 16-byte-a-lane kernels (the staged and the one-wave-a-row kernel of the forward call, the gather of
    the backward call); an x, a y, a gy or a gx one element past a 16-byte boundary must take the one-element kernels: RLAP_OK, the
    bits of the aligned call, nothing written in front of or behind the result."""
    assert F % (16 // torch.empty(0, dtype=dtype).element_size()) == 0
    x, node_ptr = small(dtype, F=F)
    L, N, G = x.shape[0], x.shape[1], node_ptr.numel() - 1
    for flags in (0, MEAN):
        rc, y0, _ = forward(env, handle, x, node_ptr, flags)
        assert rc == OK and x.data_ptr() % 16 == 0 and y0.data_ptr() % 16 == 0
        assert torch.equal(y0, exact(x, node_ptr, flags == MEAN))
        rc, gx0, _ = backward(env, handle, y0, node_ptr, N, flags)
        assert rc == OK and gx0.data_ptr() % 16 == 0 and bool((gx0 != PATTERN).all())
        for x_off, y_off in ((True, False), (False, True), (True, True)):
            xv = off_the_grid(x)[0] if x_off else x
            yv, ybig = off_the_grid(shape=(L, G, F), dtype=dtype) if y_off else (None, None)
            rc, y, _ = forward(env, handle, xv, node_ptr, flags, y=yv)
            assert rc == OK, (x_off, y_off)
            assert bits_equal(y, y0), (x_off, y_off)
            assert not y_off or around_intact(ybig, L * G * F), (x_off, y_off)
            gyv = off_the_grid(y0)[0] if x_off else y0
            gxv, gbig = off_the_grid(shape=(L, N, F), dtype=dtype) if y_off else (None, None)
            rc, gx, _ = backward(env, handle, gyv, node_ptr, N, flags, gx=gxv)
            assert rc == OK, (x_off, y_off)
            assert bits_equal(gx, gx0), (x_off, y_off)
            assert not y_off or around_intact(gbig, L * N * F), (x_off, y_off)


def test_one_graph_reports_exact_counts(env, handle):
    x, _ = small()
    rc, y, info = forward(env, handle, x, torch.tensor([0, 700]).cuda(), 0)
    assert rc == OK and (info.chunks, info.chunked_graphs) == (3, 1) and torch.equal(y, x.sum(1, keepdim=True))
    rc, y, info = forward(env, handle, x[:, :200].contiguous(), torch.tensor([0, 200]).cuda(), 0)
    assert rc == OK and (info.chunks, info.chunked_graphs) == (1, 0)


def test_host_checks_answer_before_anything_is_launched(env, handle):
    x, node_ptr = small()
    cases = [
        ({"G": 0}, BAD_ARG), ({"F": 0}, BAD_ARG), ({"flags": UNKNOWN_FLAG}, BAD_ARG), ({"flags": 2}, BAD_ARG),
        ({"L": -1}, BAD_ARG), ({"N": -1}, BAD_ARG), ({"node_ptr": None}, BAD_ARG), ({"x": None}, BAD_ARG), ({"y": None}, BAD_ARG),
        ({"F": SPMM_MAX_F + 1}, TOO_LARGE), ({"N": 1 << 40}, TOO_LARGE), ({"L": 1 << 30, "N": 1 << 12}, TOO_LARGE),
    ]
    for over, want in cases:
        flags = over.get("flags", 0)
        over = {k: v for k, v in over.items() if k != "flags"}
        rc, y, _ = forward(env, handle, x, node_ptr, flags, over=over)
        assert rc == want, over
        assert bool((y == PATTERN).all()), over
        over_b = {{"x": "gy", "y": "gx"}.get(k, k): v for k, v in over.items()}
        rc, gx, _ = backward(env, handle, exact(x, node_ptr), node_ptr, 700, flags, over=over_b)
        assert rc == want, over_b
        assert bool((gx == PATTERN).all()), over_b
    info = env["_lib"].ReadoutInfo()
    assert env["lib"].rlap_graph_readout(None, ptr(x), 2, 700, 6, ptr(node_ptr), 4, 0, ptr(x), ctypes.byref(info)) == BAD_ARG
    assert forward(env, handle, x, node_ptr, 0, over={"F": SPMM_MAX_F, "x": None, "y": None, "L": 0})[0] == OK          # the limit itself; no layer, nothing to do


def test_a_callers_arena(env, handle):
    lib = env["lib"]
    x, node_ptr = small()
    tiny = torch.empty(64, dtype=torch.uint8, device="cuda")
    rng = torch.empty(1 << 16, dtype=torch.float64, device="cuda")
    assert lib.rlap_set_workspace(handle, tiny.data_ptr(), tiny.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, y, _ = forward(env, handle, x, node_ptr, 0)
    assert rc == E_WORKSPACE and bool((y == PATTERN).all())
    need, rn = ctypes.c_size_t(0), ctypes.c_int64(0)
    assert lib.rlap_workspace_needed(handle, ctypes.byref(need), ctypes.byref(rn)) == OK and need.value > 64
    ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    assert lib.rlap_set_workspace(handle, ws.data_ptr(), ws.numel(), rng.data_ptr(), rng.numel()) == OK
    rc, y, info = forward(env, handle, x, node_ptr, 0)
    assert rc == OK and info.arena_bytes == need.value and torch.equal(y, exact(x, node_ptr))
    assert backward(env, handle, y, node_ptr, 700, MEAN)[0] == OK


@pytest.mark.parametrize("table", [[0, 9, 4, 12], [0, 5, 40], [-3, 6, 12], [7, 7, 7, 100], [0, 12, 0, 12, 0, 12]])
@pytest.mark.parametrize("F", [1, 4, 64])
def test_a_table_that_is_not_well_formed_is_clamped(env, handle, table, F):
    """num_nodes = 12: whatever the table says, no row outside x is read and no element outside y or gx written.  The buffers sit
    inside larger ones filled with a pattern; the call returns RLAP_OK, the stream synchronises cleanly and the pattern around the
    results is intact."""
    N, L = 12, 2
    G = len(table) - 1
    node_ptr = torch.tensor(table, dtype=torch.int64).cuda()
    x = torch.ones(L, N, F, dtype=torch.float64, device="cuda")
    for flags in (0, MEAN):
        big = torch.full((L * G * F + 512,), PATTERN, dtype=torch.float64, device="cuda")
        y = big[256:256 + L * G * F].view(L, G, F)
        rc, y, _ = forward(env, handle, x, node_ptr, flags, y=y)
        assert rc == OK
        assert bool((big[:256] == PATTERN).all()) and bool((big[256 + L * G * F:] == PATTERN).all())
        assert bool(torch.isfinite(y).all()) and bool((y >= 0).all()) and bool((y <= N).all())    # some numbers: sums of at most N ones
        rc, gx, _ = backward(env, handle, y.contiguous(), node_ptr, N, flags)
        assert rc == OK and gx.shape == (L, N, F) and bool((gx != PATTERN).all())                  # every element of gx is written
