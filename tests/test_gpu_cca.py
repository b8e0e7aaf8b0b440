"""The fused CCA-SSG loss on the device (ops.cca_loss, rlap_cca_loss / rlap_cca_loss_backward) against its host mirror
(tests/csrc/cca_mirror.cc around rlap_amd/csrc/rlap_cca.h, the header the kernels include).

Shapes: N at the edges of the MFMA's row pair, of the 32-row tile, of the 256-row chunk and of the part split (2, 3, 31, 32, 33, 64,
65, 255, 257, 300, and 2708 -- Cora's size: 64 parts), F at the edges of the 32-column tile, of the 64-column super tile and of the
template instances of both products (1, 2, 31, 32, 33, 64, 100, 256, 300, 512 -- 1, 2, 4, 8, 10 and 16 tiles: every instance, all
but one completely filled; 1, 3, 4 and 9 workgroups a (view, part)), in a sparse cross product, lambd cycling over 1e-3, 1, 0.  The
mirror runs once per shape (a module-wide cache) and serves every test.  The other tile counts (odd ones, whose clamped Gram tile
is computed twice and stored once; instances with dead registers; 2, 6 and 7 workgroups; a last workgroup of one or two live waves)
and the parts capped by the workgroup target are tests/test_gpu_loss_regimes.py's.

  forward    colstat, gram and the four terms equal the mirror's bit for bit (every operation is an IEEE float64 or float32 one,
             division and square root included; no neighbour is allowed).
  backward   dh1 and dh2 equal the mirror's bit for bit, with the upstream gradient 0.75.
"""
import math

import numpy as np
import pytest
import torch

import cca_mirror as cm
from util import ba_graph

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (3, 2), (31, 31), (32, 32), (33, 33), (64, 64), (65, 100), (255, 256), (257, 300), (300, 512), (300, 1), (2708, 33)]
LAMBDS = (1e-3, 1.0, 0.0)
CASES = [(n, f, LAMBDS[k % 3]) for k, (n, f) in enumerate(SHAPES)]
G_UP = 0.75


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


def views(n, f):
    return cm.views(n, f, 4000 + 7 * n + f)


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    lib = cm.build(tmp_path_factory.mktemp("cca"))
    cache = {}

    def get(n, f, lambd):
        key = (n, f, lambd)
        if key not in cache:
            a, b = views(n, f)
            cache[key] = cm.run(lib, a, b, lambd, g=G_UP)
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


def test_the_shapes_cover_the_part_split_and_several_workgroups(mirror):
    parts = {(n, f): mirror.lib.cca_parts(n, f) for n, f in SHAPES}
    groups = {f: mirror.lib.cca_pair_groups(f) for _, f in SHAPES}
    assert parts[(2, 1)] == 1 and parts[(2708, 33)] == 64 and parts[(300, 512)] == 10 and parts[(65, 100)] == 3
    assert groups[512] == 9 and groups[300] == 4 and groups[256] == 3 and groups[64] == 1
    assert sorted({(f + 31) // 32 for _, f in SHAPES}) == [1, 2, 4, 8, 10, 16]   # backward instances: 1, 1, 1, 2, 3, 4 tiles a wave


@pytest.mark.parametrize("n,f,lambd", CASES)
def test_forward_bit_for_bit(ops, mirror, n, f, lambd):
    a, b = views(n, f)
    m = mirror(n, f, lambd)
    terms, colstat, gram, _, _ = ops._cca_forward(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), float(lambd))
    st = dict(ops.last_stats)
    assert (st["rows"], st["features"], st["host_syncs"]) == (n, f, 0) and st["parts"] == mirror.lib.cca_parts(n, f)
    assert terms.dtype == torch.float64 and terms.shape == (4,) and colstat.shape == (4 * f,) and gram.shape == (2, f, f)
    print(f"n={n} F={f} lambd={lambd}: terms {terms.cpu().numpy()} mirror {m['terms']}")
    same("colstat", colstat, m["colstat"])
    same("gram", gram, m["gram"])
    same("terms", terms, m["terms"])
    loss = ops.cca_loss(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), lambd=lambd, return_terms=True)
    assert all(t.dim() == 0 and t.dtype == torch.float64 for t in loss)
    same("cca_loss", torch.stack(loss), m["terms"])
    if lambd == 0.0:
        assert bits(loss[0]) == bits(loss[1])


@pytest.mark.parametrize("n,f,lambd", CASES)
def test_gradients_bit_for_bit(ops, mirror, n, f, lambd):
    a, b = views(n, f)
    m = mirror(n, f, lambd)
    ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    loss = ops.cca_loss(ta, tb, lambd=lambd)
    loss.backward(torch.tensor(G_UP, dtype=torch.float64, device=loss.device))
    assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["rows"] == n
    assert ta.grad.dtype == torch.float32 and ta.grad.shape == (n, f)
    same("dh1", ta.grad, m["ga"])
    same("dh2", tb.grad, m["gb"])


def test_three_calls_and_a_poisoned_arena_give_the_same_bits(ops):
    a, b = (torch.from_numpy(x).cuda() for x in views(300, 100))

    def call():
        ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        terms = ops.cca_loss(ta, tb, lambd=1e-3, return_terms=True)
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
    parts = mirror.lib.cca_parts(n, f)
    assert parts == 29
    chunks, ffchunks = (n + 255) // 256, (f * f + 255) // 256
    a, b = (torch.from_numpy(x).cuda().requires_grad_(True) for x in views(n, f))
    loss = ops.cca_loss(a, b)
    assert ops.last_stats["arena_bytes"] == arena([chunks * 2 * f * 8, n * f * 4, n * f * 4, f * 8, 2 * parts * f * f * 4, 2 * f * f * 8, 2 * ffchunks * 8])
    assert ops.last_stats["host_syncs"] == 0 and math.isfinite(float(loss.detach()))
    loss.backward()
    assert ops.last_stats["arena_bytes"] == arena([chunks * 2 * f * 8, n * f * 4, n * f * 4, 2 * f * f * 4, n * f * 4, n * f * 4, 2 * f * 8, 2 * f * 8])
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all())


def test_a_constant_column_gives_a_nan_loss_and_no_error(ops):
    a, b = views(70, 9)
    a[:, 4] = 2.5
    ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    loss = ops.cca_loss(ta, tb)
    assert math.isnan(float(loss.detach()))
    loss.backward()
    assert bool(torch.isnan(ta.grad[:, 4]).all()) and ops.last_stats["host_syncs"] == 0


def test_value_errors_come_before_the_device(ops):
    x = torch.zeros(4, 3, device="cuda")
    for bad in ((x.double(), x.double(), 1e-3), (x, x[:3], 1e-3), (x, x, -1.0), (x[:1], x[:1], 1e-3), (x, x.cpu(), 1e-3),
                (torch.zeros(2, 513), torch.zeros(2, 513), 1e-3)):
        with pytest.raises(ValueError):
            ops.cca_loss(bad[0], bad[1], lambd=bad[2])


def test_cca_contrast_on_snapshot_gcn_conv(ops):
    """The public path of CCA-SSG's step: feature masking per view, two views of BA(300, 3) from one elimination call, one GCN layer
    for both, the loss of view 0 against view 1; loss.backward() reaches the layer's weight; the whole step repeats bit for bit."""
    from rlap_amd.adapters import CCAContrast, Graph, SnapshotGCNConv, drop_feature, rLapViews
    n, cin, cout = 300, 16, 32
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((n, cin)).astype(np.float32)).cuda()

    def step():
        torch.manual_seed(3)
        conv = SnapshotGCNConv(cin, cout).cuda()
        snaps = rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2).snapshots(g)
        xs = drop_feature(x, 0.2, views=2, generator=torch.Generator(device="cuda").manual_seed(7))
        assert xs.shape == (2, n, cin) and bool((xs == 0).all(dim=1).any())
        h = conv(xs, snaps)
        assert h.shape == (2, n, cout) and h.dtype == torch.float32
        contrast = CCAContrast(lambd=1e-3)
        loss = contrast(h)
        both = contrast(h[0], h[1])
        assert bits(loss) == bits(both)
        loss.backward()
        return loss.detach(), conv.weight.grad.clone(), conv.bias.grad.clone()
    l1, w1, b1 = step()
    l2, w2, b2 = step()
    assert l1.dtype == torch.float64 and math.isfinite(float(l1))
    assert bool(torch.isfinite(w1).all()) and float(w1.abs().max()) > 0 and bool(torch.isfinite(b1).all())
    assert bits(l1) == bits(l2) and bits(w1) == bits(w2) and bits(b1) == bits(b2)
