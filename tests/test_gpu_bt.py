"""The fused Barlow Twins loss on the device (ops.barlow_twins_loss, rlap_bt_loss / rlap_bt_loss_backward) against its
host mirror (tests/csrc/bt_mirror.cc around rlap_amd/csrc/rlap_bt.h, the header the kernels include).

Shapes: a sparse cross of N in {2, 3, 31, 32, 33, 64, 65, 255, 257, 300, 2708} (the edges of the MFMA's row pair, of the 32-row
tile, of the 256-row chunk and of the part split) and F in {1, 2, 3, 31, 32, 33, 64, 65, 100, 128, 129, 256, 300, 512}; lambd cycles
over None (1 / F), 1, 0 and eps over 1e-15, 1e-3, 0.  What reaches what:

  k_bt_cross<1>   F <= 64 (one super tile);  <2>  F = 65, 100, 128 (two);  <4>  F = 129, 256, 300, 512 (3, 4, 5, 8 super tiles)
  k_bt_zr<1>      F <= 128;  <2>  F = 129, 256;  <3>  F = 300;  <4>  F = 512
  clamped tile    F = 65 (3 tiles) and F = 129 (5 tiles): an odd Fp / 32
  block rows with fewer than four pairs    F = 129 (three), F = 300 (four and one), every F <= 128 (one or two)
  several workgroups a part                F = 256 (4), 300 (10), 512 (16)
  parts           one at N <= 32; (65, 65) 3, (257, 300) 9, (300, 512) 10 -- one per 32-row tile --; (2708, 33) 64, the cap
(300, 512) and (2708, 33) are the largest.  The mirror runs once per shape (a module-wide cache) and serves every test.

  forward    colstat, cross and the three terms equal the mirror's bit for bit (every operation is an IEEE float64 or float32 one,
             division and square root included; no neighbour is allowed).
  backward   dh1 and dh2 equal the mirror's bit for bit, with the upstream gradient 0.75.
"""
import math

import numpy as np
import pytest
import torch

import bt_mirror as bm
from util import ba_graph

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (3, 2), (31, 31), (32, 32), (33, 3), (64, 64), (65, 65), (65, 100), (255, 128), (257, 129), (300, 256), (257, 300),
          (300, 512), (300, 1), (2708, 33)]
LAMBDS = (None, 1.0, 0.0)
EPS = (1e-15, 1e-3, 0.0)
CASES = [(n, f, LAMBDS[k % 3], EPS[(k // 3) % 3]) for k, (n, f) in enumerate(SHAPES)]
G_UP = 0.75


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


def views(n, f):
    return bm.views(n, f, 4000 + 7 * n + f)


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    lib = bm.build(tmp_path_factory.mktemp("bt"))
    cache = {}

    def get(n, f, lambd, eps, standardize=True):
        key = (n, f, lambd, eps, standardize)
        if key not in cache:
            a, b = views(n, f)
            cache[key] = bm.run(lib, a, b, lambd, eps, standardize, g=G_UP)
        return cache[key]
    get.lib = lib
    return get


def bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).tobytes()


def where(got, want):
    """Where two arrays differ, for the message of a failed comparison of bits."""
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return " (in the sign of a zero or in a NaN)"
    i = tuple(bad[0])
    return f": {len(bad)} elements differ, first at {i}: {got[i]!r} != {want[i]!r}"


def same(name, got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert bits(got) == bits(want), name + where(got, want)


def dev(x):
    return torch.from_numpy(x).cuda()


def test_the_shapes_cover_the_instances_the_work_map_and_the_parts(mirror):
    lib = mirror.lib
    parts = {(n, f): lib.bt_parts(n, f) for n, f in SHAPES}
    assert parts[(2, 1)] == 1 and parts[(32, 32)] == 1 and parts[(65, 65)] == 3 and parts[(257, 300)] == 9 and parts[(300, 512)] == 10
    assert parts[(2708, 33)] == 64                                            # the cap: 85 row tiles, one workgroup a part
    fs = sorted({f for _, f in SHAPES})
    assert {lib.bt_cross_instance(lib.bt_feature_tiles(f)) for f in fs} == {1, 2, 4}
    assert {lib.bt_zr_instance(lib.bt_feature_tiles(f)) for f in fs} == {1, 2, 3, 4}
    assert [f for f in fs if lib.bt_feature_tiles(f) % 2 == 1 and f > 32] == [65, 129]              # the clamped tile
    assert {f: lib.bt_pair_groups(f) for f in (128, 129, 256, 300, 512)} == {128: 2, 129: 3, 256: 4, 300: 10, 512: 16}
    assert {f: lib.bt_row_groups(f) for f in (129, 256, 300, 512)} == {129: 1, 256: 1, 300: 2, 512: 2}   # 3 | 4 | 4 + 1 | 4 + 4 pairs a row
    assert sorted({n for n, _ in SHAPES}) == [2, 3, 31, 32, 33, 64, 65, 255, 257, 300, 2708]
    assert fs == [1, 2, 3, 31, 32, 33, 64, 65, 100, 128, 129, 256, 300, 512]


@pytest.mark.parametrize("n,f,lambd,eps", CASES)
def test_forward_bit_for_bit(ops, mirror, n, f, lambd, eps):
    a, b = views(n, f)
    m = mirror(n, f, lambd, eps)
    terms, colstat, cross, _, _ = ops._bt_forward(dev(a), dev(b), bm.lambd_of(lambd, f), eps, 0)
    st = dict(ops.last_stats)
    assert (st["rows"], st["features"], st["host_syncs"]) == (n, f, 0) and st["parts"] == mirror.lib.bt_parts(n, f)
    assert terms.dtype == torch.float64 and terms.shape == (3,) and colstat.shape == (4 * f,) and cross.shape == (f, f)
    print(f"n={n} F={f} lambd={lambd} eps={eps}: terms {terms.cpu().numpy()} mirror {m['terms']}")
    same("colstat", colstat, m["colstat"])
    same("cross", cross, m["cross"])
    same("terms", terms, m["terms"])
    loss = ops.barlow_twins_loss(dev(a), dev(b), lambd=lambd, eps=eps, return_terms=True)
    assert all(t.dim() == 0 and t.dtype == torch.float64 for t in loss)
    same("barlow_twins_loss", torch.stack(loss), m["terms"])
    if lambd == 0.0:
        assert bits(loss[0]) == bits(loss[1])
    if n >= 31 and f >= 3:
        c = cross.cpu().numpy()
        assert np.abs(c - c.T).max() >= 0.5                                   # not a symmetric matrix: a transposed kernel fails above


@pytest.mark.parametrize("n,f,lambd,eps", CASES)
def test_gradients_bit_for_bit(ops, mirror, n, f, lambd, eps):
    a, b = views(n, f)
    m = mirror(n, f, lambd, eps)
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    loss = ops.barlow_twins_loss(ta, tb, lambd=lambd, eps=eps)
    loss.backward(torch.tensor(G_UP, dtype=torch.float64, device=loss.device))
    assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["rows"] == n
    assert ta.grad.dtype == torch.float32 and ta.grad.shape == (n, f)
    same("dh1", ta.grad, m["ga"])
    same("dh2", tb.grad, m["gb"])


@pytest.mark.parametrize("n,f", [(65, 65), (257, 129)])
def test_without_the_standardisation(ops, mirror, n, f):
    a, b = views(n, f)
    m = mirror(n, f, None, 1e-15, False)
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    terms = ops.barlow_twins_loss(ta, tb, standardize=False, return_terms=True)
    terms[0].backward(torch.tensor(G_UP, dtype=torch.float64, device="cuda"))
    same("terms", torch.stack([t.detach() for t in terms]), m["terms"])
    same("dh1", ta.grad, m["ga"])
    same("dh2", tb.grad, m["gb"])
    fill = torch.full((4 * f,), -7.25, dtype=torch.float64, device="cuda")    # colstat is not written
    out = torch.empty(3, dtype=torch.float64, device="cuda")
    cross = torch.empty(f, f, device="cuda")
    ops._device_call("rlap_bt_loss", ops._lib.BtInfo, ta.device, 1, (ta.data_ptr(), tb.data_ptr(), n, f, 1.0 / f, 1e-15, 1, out.data_ptr(),
                                                                     fill.data_ptr(), cross.data_ptr()))
    assert bool((fill == -7.25).all())
    same("terms", out, m["terms"])
    same("cross", cross, m["cross"])


def test_three_calls_and_a_poisoned_arena_give_the_same_bits(ops):
    a, b = (dev(x) for x in views(300, 100))

    def call():
        ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        terms = ops.barlow_twins_loss(ta, tb, return_terms=True)
        terms[0].backward()
        return [bits(t) for t in (*terms, ta.grad, tb.grad)]
    base = call()
    assert call() == base and call() == base
    for byte in (0xFF, 0x00, 0x3C):
        ops.debug_set_poison(byte)
        try:
            assert call() == base, f"poison {byte:#x}"
        finally:
            ops.debug_set_poison(-1)
    assert ops.last_stats["host_syncs"] == 0


def r256(x):
    return (x + 255) // 256 * 256


def arena(sizes):
    off = 0
    for s in sizes:
        off = r256(off) + s
    return off + 256


def test_the_arena_is_the_formula_of_the_design(ops, mirror):
    n, f = 4096, 512
    parts = mirror.lib.bt_parts(n, f)
    assert parts == 16
    chunks, ffchunks, fchunks = (n + 255) // 256, (f * f + 255) // 256, (f + 255) // 256
    a, b = (dev(x).requires_grad_(True) for x in views(n, f))
    loss = ops.barlow_twins_loss(a, b)
    assert ops.last_stats["arena_bytes"] == arena([chunks * 2 * f * 8, n * f * 4, n * f * 4, parts * f * f * 4, f * f * 8, (ffchunks + fchunks) * 8])
    assert ops.last_stats["host_syncs"] == 0 and math.isfinite(float(loss.detach()))
    loss.backward()
    assert ops.last_stats["arena_bytes"] == arena([chunks * 2 * f * 8, n * f * 4, n * f * 4, 2 * f * f * 4, n * f * 4, n * f * 4, 2 * f * 8, 2 * f * 8])
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all())


def nan_aware(name, got, want):
    """Equal bits wherever the mirror is not NaN, NaN wherever it is (the payload of a NaN is the processor's)."""
    got = got.detach().cpu().numpy()
    assert (np.isnan(got) == np.isnan(want)).all(), name
    keep = ~np.isnan(want)
    assert bits(got[keep]) == bits(want[keep]), name + where(got[keep], want[keep])


@pytest.mark.parametrize("eps", [1e-15, 0.0])
def test_a_constant_column_agrees_with_the_mirror(ops, mirror, eps):
    a, b = views(70, 9)
    a[:, 4] = 2.5
    m = bm.run(mirror.lib, a, b, eps=eps, g=G_UP)
    ta, tb = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    terms = ops.barlow_twins_loss(ta, tb, eps=eps, return_terms=True)
    terms[0].backward(torch.tensor(G_UP, dtype=torch.float64, device="cuda"))
    assert ops.last_stats["host_syncs"] == 0
    nan_aware("terms", torch.stack([t.detach() for t in terms]), m["terms"])
    nan_aware("dh1", ta.grad, m["ga"])
    nan_aware("dh2", tb.grad, m["gb"])
    assert math.isfinite(float(terms[0].detach())) == (eps > 0) and bool(torch.isnan(ta.grad[:, 4]).all())
    if eps > 0:
        assert bool(torch.isfinite(tb.grad).all()) and int(torch.isnan(ta.grad).sum()) == 70


def test_value_errors_come_before_the_device(ops):
    x = torch.zeros(4, 3, device="cuda")
    for bad in ((x.double(), x.double(), {}), (x, x[:3], {}), (x, x, {"lambd": -1.0}), (x, x, {"eps": -1.0}), (x[:1], x[:1], {}), (x, x.cpu(), {}),
                (torch.zeros(2, 513), torch.zeros(2, 513), {}), (x, x, {"standardize": 0})):
        with pytest.raises(ValueError):
            ops.barlow_twins_loss(bad[0], bad[1], **bad[2])


def test_barlow_twins_contrast_on_snapshot_gcn_conv(ops):
    """The public path of a G-BT step: feature masking per view, two views of BA(300, 3) from one elimination call, one GCN layer
    for both, the loss of view 0 against view 1; loss.backward() reaches the layer's weight; the whole step repeats bit for bit."""
    from rlap_amd.adapters import BarlowTwinsContrast, Graph, SnapshotGCNConv, drop_feature, rLapViews
    n, cin, cout = 300, 16, 32
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((n, cin)).astype(np.float32)).cuda()

    def step():
        torch.manual_seed(3)
        conv = SnapshotGCNConv(cin, cout).cuda()
        snaps = rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2).snapshots(g)
        xs = drop_feature(x, 0.2, views=2, generator=torch.Generator(device="cuda").manual_seed(7))
        h = conv(xs, snaps)
        assert h.shape == (2, n, cout) and h.dtype == torch.float32
        contrast = BarlowTwinsContrast()
        loss = contrast(h)
        both = contrast(h[0], h[1])
        assert bits(loss) == bits(both)
        assert bits(loss) == bits(ops.barlow_twins_loss(h[0], h[1], lambd=1.0 / cout))
        loss.backward()
        return loss.detach(), conv.weight.grad.clone(), conv.bias.grad.clone()
    l1, w1, b1 = step()
    l2, w2, b2 = step()
    assert l1.dtype == torch.float64 and math.isfinite(float(l1))
    assert bool(torch.isfinite(w1).all()) and float(w1.abs().max()) > 0 and bool(torch.isfinite(b1).all())
    assert bits(l1) == bits(l2) and bits(w1) == bits(w2) and bits(b1) == bits(b2)
