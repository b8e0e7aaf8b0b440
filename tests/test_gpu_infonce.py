"""The fused InfoNCE loss on the device (ops.info_nce, rlap_infonce / rlap_infonce_backward) against its host mirror
(tests/csrc/infonce_mirror.cc around rlap_amd/csrc/rlap_infonce.h, the header the kernels include).

Shapes: N at the edges of the 32-wide tiles, of the workgroup's 128-row block and of the part split (1, 31, 32, 33, 64, 65, 127, 129,
300, and 2708 -- Cora's size: several parts, many workgroups), F at the edges of the MFMA's k pair, of the 8-column fragment group
and of the 32-column feature tiles of the backward accumulators (1, 2, 3, 31, 32, 33, 100, 256, 512 -- 1, 2, 4, 8 and 16 tiles:
every template instance, each completely filled), in a sparse cross product.  The mirror runs once per shape (a module-wide cache)
and serves every test.  The other tile counts (an instance with dead accumulator tiles), the part counts below the tile count and
the single part of N >= 32,641 are tests/test_gpu_loss_regimes.py's.

  forward    Z equals the mirror's bit for bit.  rows: the device's float64 log may differ from the host's by one unit in the last
             place and nothing else may, so with u = c s_ii - 1/tau from the MIRROR's s_ii, the device's row must be fl(u - L) for L
             one of log(Z) and its two neighbours, bit for bit -- which pins s_ii's bits --, and lie within 1e-13 of the mirror's;
             the loss within 1e-13.
  backward   ga and gb equal the mirror's bit for bit.
  operands   rows of one 1 (anchors) and of four +-1 (samples: +-0.5 after the normalisation) make every s_ij exactly 0 or +-0.5 with
             an asymmetric pattern; Z_i is then a count of three values of expw whose float64 sum is exact in any order, and a
             row / column swap changes the counts.
"""
import math

import numpy as np
import pytest
import torch

import infonce_mirror as im
from util import ba_graph

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (31, 2), (32, 3), (33, 31), (64, 32), (65, 33), (127, 100), (129, 256), (300, 512), (300, 1), (2708, 33)]
CASES = [(n, f, ("scaled", "raw")[k % 2], (0.4, 1.0 / 32.0, 2.0)[k % 3]) for k, (n, f) in enumerate(SHAPES)]
G_UP = 0.75


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    lib = im.build(tmp_path_factory.mktemp("infonce"))
    cache = {}

    def get(n, f, positive, tau):
        key = (n, f, positive, tau)
        if key not in cache:
            a, b = views(n, f)
            cache[key] = im.run(lib, a, b, tau, positive, g=G_UP)
        return cache[key]
    get.lib = lib
    return get


def views(n, f, seed=None):
    rng = np.random.RandomState(4000 + 7 * n + f if seed is None else seed)
    a = rng.standard_normal((n, f)).astype(np.float32)
    b = (0.3 * a + rng.standard_normal((n, f))).astype(np.float32)
    return a, b


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


@pytest.mark.parametrize("n,f,positive,tau", CASES)
def test_forward_against_the_mirror(ops, mirror, n, f, positive, tau):
    a, b = views(n, f)
    m = mirror(n, f, positive, tau)
    loss, rows = ops.info_nce(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), tau=tau, positive=positive, return_rows=True)
    st = dict(ops.last_stats)
    assert (st["rows"], st["features"], st["host_syncs"]) == (n, f, 0) and st["parts"] == mirror.lib.infonce_parts(n)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and rows.shape == (n,)
    err = rows_against_the_mirror(rows, m, positive, tau)
    print(f"n={n} F={f} {positive} tau={tau}: rows max |diff| {err:.3g}, loss diff {abs(float(loss) - m['loss']):.3g}")
    assert err <= 1e-13
    assert abs(float(loss) - m["loss"]) <= 1e-13


def rows_against_the_mirror(rows, m, positive, tau):
    """Asserts the neighbour rule of the module docstring on the device's rows (every row is fl(u - L), u from the mirror's s_ii and L
    one of log(Z) and its two neighbours); returns the largest |row - the mirror's row|, which the caller holds to 1e-13."""
    rows = rows.cpu().numpy()
    c = 1.0 if positive == "raw" else 1.0 / tau
    u = c * m["sii"].astype(np.float64) - 1.0 / tau
    L = np.log(m["z"])
    allowed = np.stack([u - np.nextafter(L, -np.inf), u - L, u - np.nextafter(L, np.inf)])
    assert (rows[None, :] == allowed).any(axis=0).all(), "a row is not c s_ii - 1/tau - log Z with the mirror's s_ii and Z"
    return np.abs(rows - m["rows"]).max()


@pytest.mark.parametrize("n,f,positive,tau", CASES)
def test_row_sums_and_gradients_bit_for_bit(ops, mirror, n, f, positive, tau):
    a, b = views(n, f)
    m = mirror(n, f, positive, tau)
    ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    z = forward_z(ops, ta.detach(), tb.detach(), tau, positive)
    assert bits(z) == bits(m["z"]), "Z" + where(z.cpu().numpy(), m["z"])
    loss = ops.info_nce(ta, tb, tau=tau, positive=positive)
    loss.backward(torch.tensor(G_UP, dtype=torch.float64, device=loss.device))
    assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["rows"] == n
    assert ta.grad.dtype == torch.float32 and ta.grad.shape == (n, f)
    assert bits(ta.grad) == bits(m["ga"]), "ga" + where(ta.grad.cpu().numpy(), m["ga"])
    assert bits(tb.grad) == bits(m["gb"]), "gb" + where(tb.grad.cpu().numpy(), m["gb"])


def forward_z(ops, a, b, tau, positive):
    """The row sums Z of the forward export (its third result, which ops keeps for the backward call)."""
    return ops._info_nce_forward(a, b, float(tau), ops.INFONCE_POSITIVE[positive])[2]


def exact_views(n, f):
    """The data of test_operand_maps_with_exact_data: a_i = e_(i mod F), b_j = four entries +-1 in columns drawn per j."""
    rng = np.random.RandomState(n + f)
    a = np.zeros((n, f), dtype=np.float32)
    a[np.arange(n), np.arange(n) % f] = 1.0
    b = np.zeros((n, f), dtype=np.float32)
    for j in range(n):
        b[j, rng.choice(f, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    return a, b


@pytest.mark.parametrize("n,f", [(65, 8), (300, 40), (129, 33)])
def test_operand_maps_with_exact_data(ops, mirror, n, f):
    """a_i = e_(i mod F); b_j = four entries +-1 (hat: +-0.5) in columns drawn per j: s_ij = bh_j[i mod F], exactly 0 or +-0.5, and
    s_ij != s_ji in general.  Z_i = (count of +0.5) e+ + (count of 0) e0 + (count of -0.5) e-, exact in float64 in any order."""
    tau = 2.0
    a, b = exact_views(n, f)
    s = (b / 2.0)[:, np.arange(n) % f].T                                        # s[i, j] = bh_j[i mod F]
    assert not np.array_equal(s, s.T)
    itf = np.float32(1.0 / tau)
    e = {v: np.float64(im.expw(mirror.lib, np.array([(np.float32(v) - np.float32(1.0)) * itf], dtype=np.float32))[0]) for v in (-0.5, 0.0, 0.5)}
    z_want = sum((s == v).sum(axis=1) * e[v] for v in (-0.5, 0.0, 0.5))
    z_swapped = sum((s.T == v).sum(axis=1) * e[v] for v in (-0.5, 0.0, 0.5))
    assert not np.array_equal(z_want, z_swapped)                                # a row / column swap would show
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    z = forward_z(ops, ta, tb, tau, "raw").cpu().numpy()
    assert bits(z) == bits(z_want), "Z" + where(z, z_want)
    rows = ops.info_nce(ta, tb, tau=tau, positive="raw", return_rows=True)[1].cpu().numpy()
    want = 1.0 * np.diag(s) - 1.0 / tau - np.log(z_want)
    assert np.abs(rows - want).max() <= 1e-13                                   # s_ii exact: diag(s), not a neighbour's
    # the second products: the mirror's bits on the same data
    m = im.run(mirror.lib, a, b, tau, "raw", g=1.0)
    ta.requires_grad_(True)
    tb.requires_grad_(True)
    ops.info_nce(ta, tb, tau=tau, positive="raw").backward()
    assert bits(ta.grad) == bits(m["ga"]) and bits(tb.grad) == bits(m["gb"])


def test_two_calls_and_a_poisoned_arena_give_the_same_bits(ops):
    a, b = (torch.from_numpy(x).cuda() for x in views(300, 100))

    def call():
        ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        loss, rows = ops.info_nce(ta, tb, tau=0.4, positive="raw", return_rows=True)
        loss.backward()
        return [bits(t) for t in (loss, rows, ta.grad, tb.grad)]
    base = call()
    assert call() == base
    for byte in (0xFF, 0x00, 0x3C):
        ops.debug_set_poison(byte)
        try:
            assert call() == base, f"poison {byte:#x}"
        finally:
            ops.debug_set_poison(-1)
    assert ops.last_stats["host_syncs"] == 0


def test_memory_is_linear_in_n(ops):
    n, f = 4096, 64
    a, b = (torch.from_numpy(x).cuda() for x in views(n, f))
    loss = ops.info_nce(a, b)
    assert ops.last_stats["arena_bytes"] < n * n * 4 // 8 and ops.last_stats["host_syncs"] == 0
    assert math.isfinite(float(loss))


def test_zero_rows_and_the_ends_of_tau(ops, mirror):
    a, b = views(70, 9, seed=3)
    a[5] = 0.0
    b[40] = 0.0
    for tau in (1.0 / 32.0, 1024.0):
        m = im.run(mirror.lib, a, b, tau, "scaled", g=1.0)
        ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
        loss = ops.info_nce(ta, tb, tau=tau)
        loss.backward()
        assert abs(float(loss.detach()) - m["loss"]) <= 1e-13 and bits(ta.grad) == bits(m["ga"]) and bits(tb.grad) == bits(m["gb"])
        assert bool(torch.isfinite(ta.grad).all()) and bool(torch.isfinite(tb.grad).all())


def test_value_errors_come_before_the_device(ops):
    x = torch.zeros(4, 3, device="cuda")
    for bad in ((x.double(), x.double(), 0.4), (x, x[:3], 0.4), (x, x, 0.0), (torch.zeros(2, 513), torch.zeros(2, 513), 0.4)):
        with pytest.raises(ValueError):
            ops.info_nce(bad[0], bad[1], tau=bad[2])


def test_node_contrast_on_snapshot_gcn_conv(ops):
    """The public path of the node-level step: two views of BA(300, 3) from one elimination call, one GCN layer for both, the
    contrastive loss of view 0 against view 1; loss.backward() reaches the layer's weight; the whole step repeats bit for bit."""
    from rlap_amd.adapters import Graph, NodeContrast, SnapshotGCNConv, rLapViews
    n, cin, cout = 300, 16, 32
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((n, cin)).astype(np.float32)).cuda()

    def step():
        torch.manual_seed(3)
        conv = SnapshotGCNConv(cin, cout).cuda()
        snaps = rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2).snapshots(g)
        h = conv(x, snaps)
        assert h.shape == (2, n, cout) and h.dtype == torch.float32
        contrast = NodeContrast(tau=0.4)
        loss = contrast(h)
        both = contrast(h[0], h[1])
        assert bits(loss) == bits(both)
        loss.backward()
        return loss.detach(), conv.weight.grad.clone(), conv.bias.grad.clone()
    l1, w1, b1 = step()
    l2, w2, b2 = step()
    assert l1.dtype == torch.float64 and math.isfinite(float(l1)) and float(l1) > 0
    assert bool(torch.isfinite(w1).all()) and float(w1.abs().max()) > 0 and bool(torch.isfinite(b1).all())
    assert bits(l1) == bits(l2) and bits(w1) == bits(w2) and bits(b1) == bits(b2)
