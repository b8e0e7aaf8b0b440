"""The sparse first layer's kernels stride over their tasks under a cap of 2^20 workgroups of 256 threads (FL_MAX_GRID in
rlap_amd/csrc/rlap_featlin.hip).  A slot takes 64 lanes at Fout = 256 float32 (one 16-byte load a lane), so 2^22 slots fill the
grid once and 65 more reach the second round: N = 2^22 + 65 rows for the forward launch, Fin = 2^22 + 65 columns for the transposed
row launch.  Each case is compared with the float64 product in torch on the device within the bound of tests/test_featlin_cpu.py,
and bit for bit with the host mirror on the first 300 slots, the last 300 and the 300 around 2^22 (slots are independent, so the
mirror runs on the sub-matrix of those slots)."""
import numpy as np
import pytest
import torch

import featlin_mirror as fm
from test_gpu_propagate import bound_factor

pytestmark = pytest.mark.gpu

BIG, SMALL, FOUT = 2 ** 22 + 65, 8, 256
# the first 300 slots, the 300 around 2^22 as far as there are slots, the last 300 (the two overlap: 2^22 is 65 slots from the end)
SLOTS = np.unique(np.concatenate([np.arange(300), np.arange(2 ** 22 - 150, min(2 ** 22 + 150, BIG)), np.arange(BIG - 300, BIG)]))
assert SLOTS.min() == 0 and SLOTS.max() == BIG - 1
BLOCK = 2 ** 19


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return fm.build(tmp_path_factory.mktemp("featlin"))


def sparse_on_device(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(shape, generator=g, device="cuda") + 0.25
    return x * (torch.rand(shape, generator=g, device="cuda") < 0.3)


def worst_ratio(y, ref, A, factor):
    bound = factor * A
    bound = bound + 2.0 ** -24 * (ref.abs() + bound)
    err = (y.double() - ref).abs()
    assert bool((y[A == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max())


def test_forward_rows_reach_the_second_round(mirror):
    from rlap_amd import ops
    x = sparse_on_device((BIG, SMALL), 1)
    fp = ops.feature_plan(x, "forward")
    assert fp.info["longest_forward"] <= SMALL and fp.info["chunks_forward"] == 0
    w = torch.rand((SMALL, FOUT), generator=torch.Generator(device="cuda").manual_seed(2), device="cuda") - 0.5
    y = fp.linear(w)
    assert y.shape == (BIG, FOUT) and (BIG * 64 + 255) // 256 > 2 ** 20
    worst = 0.0
    for r0 in range(0, BIG, BLOCK):
        xb = x[r0:r0 + BLOCK].double()
        worst = max(worst, worst_ratio(y[r0:r0 + BLOCK], xb @ w.double(), xb.abs() @ w.double().abs(), bound_factor(SMALL, True)))
    print(f"forward, {BIG} rows: worst |y - ref| / bound = {worst:.3e}")
    assert worst <= 1.0
    sel = torch.from_numpy(SLOTS).cuda()
    p = fm.plan(mirror, x[sel].cpu().numpy(), "forward")
    assert fm.same_bits(y[sel].cpu().numpy(), fm.apply(mirror, p, w.cpu().numpy())[0])


def test_transposed_columns_reach_the_second_round(mirror):
    from rlap_amd import ops
    x = sparse_on_device((SMALL, BIG), 3)
    fp = ops.feature_plan(x, "transposed")
    assert fp.info["longest_transposed"] <= SMALL and fp.info["chunks_transposed"] == 0
    g = torch.rand((1, SMALL, FOUT), generator=torch.Generator(device="cuda").manual_seed(4), device="cuda") - 0.5
    dw = ops._feature_apply(fp, g, None, 1, True)
    assert dw.shape == (BIG, FOUT)
    worst = 0.0
    for c0 in range(0, BIG, BLOCK):
        xb = x[:, c0:c0 + BLOCK].double().t()
        worst = max(worst, worst_ratio(dw[c0:c0 + BLOCK], xb @ g[0].double(), xb.abs() @ g[0].double().abs(), bound_factor(SMALL, True)))
    print(f"transposed, {BIG} columns: worst |dW - ref| / bound = {worst:.3e}")
    assert worst <= 1.0
    sel = torch.from_numpy(SLOTS).cuda()
    p = fm.plan(mirror, x[:, sel].cpu().numpy(), "transposed")
    assert fm.same_bits(dw[sel].cpu().numpy(), fm.apply(mirror, p, g.cpu().numpy(), transpose=True))
