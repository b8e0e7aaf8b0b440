"""The lane paths of the planned call (rlap_plan.hip's launch_sums: k_pl_rows / k_pl_chunks as <T, 4>, <T, 2> and <T, 1>) at the
feature widths the other suites leave out, and the alignment fallback of the planned and the unplanned call.

F_PATHS (tests/test_gpu_propagate.py says which path each width takes) runs the one-column kernels with two and three tiles of
lanes, a vector kernel whose second tile holds one lane, groups with idle lanes and one exactly full tile.  Every comparison is
bits: with the unplanned call, and -- independently of it -- with the host mirror of rlap_spmm.h fed with the float64 coefficients
of ops.snapshot_gcn_norm; a float32 result is the mirror's float64 result of x32.double() rounded once.

The fallback: F a multiple of the lanes' vector width, but x one element into a larger buffer, so its address is no multiple of
16 bytes although the tensor is contiguous (ops passes such a view on as it is).  launch_sums must then take the one-column
kernels; the result has the bits of the same call on an aligned copy.

Every call here runs under debug_set_poison(0xFF): y holds NaN patterns before the call, so a tile of lanes that is never written
cannot pass by finding an earlier call's result in reused memory."""
import numpy as np
import pytest
import torch

from test_gpu_plan import depths_views, features, mirror, ops, same, two_stars  # noqa: F401  (mirror, ops are fixtures)
from test_gpu_propagate import F_PATHS, mirror_result, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def poisoned(ops):
    ops.debug_set_poison(0xFF)
    yield
    ops.debug_set_poison(-1)


KW = {"weighted": True}


def inputs(ops, mirror, which):
    if which == "depths":
        n = 300
        sc, ptr = depths_views(ops, n, 3, 2, "random", [75, 150], views=2)
        return sc, ptr, n, 0
    C = mirror.spmm_chunk()
    sc, ptr, n = two_stars(2 * C + 40)
    return sc, ptr, n, 6


def check_paths(ops, mirror, sc, ptr, n, F, what):
    plan = ops.snapshot_plan(sc, ptr, n, **KW)
    L = plan.layers
    for per_layer in (False, True):
        x64 = features(n, F, L if per_layer else None)
        x32 = x64.float()
        for transpose in (False, True):
            tag = f"{what} F={F} {'per-layer' if per_layer else 'shared'} {'T' if transpose else 'N'}"
            y64 = plan.propagate(x64, transpose=transpose)
            assert ops.last_stats["host_syncs"] == 0 and y64.shape == (L, n, F), tag
            assert same(y64, ops.snapshot_propagate(sc, ptr, n, x64, transpose=transpose, **KW)), f"{tag}: float64 differs from the unplanned call"
            want = mirror_result(ops, mirror, sc, ptr, n, x64, transpose=transpose, **KW)
            assert same_bits(y64, want), f"{tag}: float64 differs from the host mirror"
            y32 = plan.propagate(x32, transpose=transpose)
            assert same(y32, ops.snapshot_propagate(sc, ptr, n, x32, transpose=transpose, **KW)), f"{tag}: float32 differs from the unplanned call"
            want32 = mirror_result(ops, mirror, sc, ptr, n, x32.double(), transpose=transpose, **KW).float()
            assert y32.dtype == torch.float32 and same_bits(y32, want32), f"{tag}: float32 is not the mirror's float64 sum rounded once"
    return plan


@pytest.mark.parametrize("F", F_PATHS)
def test_planned_lane_paths_depths_views(ops, mirror, F):
    sc, ptr, n, _ = inputs(ops, mirror, "depths")
    check_paths(ops, mirror, sc, ptr, n, F, "depths x views")


@pytest.mark.parametrize("limit", [None, 0])
@pytest.mark.parametrize("F", F_PATHS)
def test_planned_lane_paths_long_lists(ops, mirror, F, limit):
    """Two stars of three chunks each, so that k_pl_chunks runs on every lane path; with no chunk sum kept (limit 0) k_pl_rows sums
    the long lists chunk by chunk itself."""
    sc, ptr, n, chunks = inputs(ops, mirror, "stars")
    try:
        if limit is not None:
            ops.debug_set_limits(scratch_entries=limit)
        plan = check_paths(ops, mirror, sc, ptr, n, F, f"stars limit={limit}")
        assert plan.desc.chunks_forward == chunks and plan.desc.chunks_transposed == chunks
    finally:
        ops.debug_set_limits()


def one_element_in(shape, dtype, seed):
    """(x, its aligned copy): x a contiguous view one element into a larger buffer."""
    count = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    big = torch.empty(count + 8, dtype=dtype, device="cuda")
    assert big.data_ptr() % 16 == 0
    big[1:1 + count] = torch.randn(count, dtype=torch.float64, generator=g).to(dtype).cuda()
    x = big[1:1 + count].view(shape)
    copy = x.clone()
    # the conditions of the test: without them it tests nothing
    assert x.is_contiguous() and x.data_ptr() % 16 != 0 and x.data_ptr() % x.element_size() == 0
    assert x.detach().to(device=x.device).contiguous().data_ptr() == x.data_ptr(), "the view is passed on as it is"
    assert copy.data_ptr() % 16 == 0 and torch.equal(copy, x)
    return x, copy


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("F", [16, 64, 200])
@pytest.mark.parametrize("which", ["depths", "stars"])
def test_alignment_fallback(ops, mirror, which, F, dtype):
    sc, ptr, n, _ = inputs(ops, mirror, which)
    assert F % (16 // torch.empty(0, dtype=dtype).element_size()) == 0
    plan = ops.snapshot_plan(sc, ptr, n, **KW)
    for per_layer in (False, True):
        x, copy = one_element_in((plan.layers, n, F) if per_layer else (n, F), dtype, seed=F + per_layer)
        for transpose in (False, True):
            tag = f"{which} F={F} {dtype} {'per-layer' if per_layer else 'shared'} {'T' if transpose else 'N'}"
            assert same(plan.propagate(x, transpose=transpose), plan.propagate(copy, transpose=transpose)), f"{tag}: planned"
            assert same(ops.snapshot_propagate(sc, ptr, n, x, transpose=transpose, **KW),
                        ops.snapshot_propagate(sc, ptr, n, copy, transpose=transpose, **KW)), f"{tag}: unplanned"
