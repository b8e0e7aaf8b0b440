"""The symmetric InfoNCE pair on the device (ops.info_nce_pair, rlap_infonce_pair / rlap_infonce_pair_backward) against
its host mirror (tests/csrc/infonce_pair_mirror.cc around rlap_amd/csrc/rlap_infonce.h, the header the kernels include).

Shapes, each the smallest that hits its place: N = 1, 31, 32, 33 (the tile's edge: masked owner rows and stream columns), 127, 128,
129 (the row block's edge: inactive waves in the last block, which must still reach every barrier), 300 (several parts), 2708 (22
row blocks in 16 groups: groups of one and of two blocks), 4133 (33 row blocks: groups of two and three); F in {1, 3, 32, 33, 100,
256, 512} paired with them, F <= 33 at the two largest N so that the mirror stays within seconds.  The mirror runs once per shape.

  forward    Z and Zc equal the mirror's bit for bit.  Each row term is fl(u - L) with u = c s_ii - 1/tau from the MIRROR's s_ii and L
             one of log(Z) and its two neighbours (the rule of tests/test_gpu_infonce.py), within 1e-13 of the mirror's; the loss
             within 1e-13.
  backward   ga and gb equal the mirror's bit for bit.
  operands   exact data: rows of one 1 (anchors) and of four +-1 (samples: +-0.5 after the normalisation) make every s_ij exactly 0
             or +-0.5 with S != S^T; Z_i and Zc_j are counts of three values of expw whose float64 sums are exact in any order, and
             differ from each other by a wide margin: a swap of rows and columns, or of the two reciprocals, cannot pass.
  two calls  on the device, the pair against 0.5 * (info_nce(a, b) + info_nce(b, a)) and its gradients, within the bounds measured
             between the mirrors on the CPU (tests/test_infonce_pair_cpu.py has the figures and the reasoning).
"""
import math

import numpy as np
import pytest
import torch

import infonce_mirror as im
import infonce_pair_mirror as pm
from util import ba_graph

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (31, 3), (32, 32), (33, 33), (127, 100), (128, 256), (129, 512), (300, 256), (300, 1), (2708, 33), (4133, 3)]
CASES = [(n, f, ("scaled", "raw")[k % 2], (0.4, 1.0 / 32.0, 2.0)[k % 3]) for k, (n, f) in enumerate(SHAPES)]
G_UP = 0.75
PAIR_GRAD_BOUND = 4 * 1.05e-6     # of the largest gradient entry: measured between the mirrors (tests/test_infonce_pair_cpu.py)


def pair_loss_abs(n):
    """The float64 bound on |pair - two calls| of tests/test_infonce_pair_cpu.py's docstring."""
    return (n + 256) * 2.0 ** -52


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    lib = pm.build(tmp_path_factory.mktemp("infonce_pair"))
    lib1 = im.build(tmp_path_factory.mktemp("infonce_one"))      # the one-direction mirror: its expw export
    cache = {}

    def get(n, f, positive, tau):
        key = (n, f, positive, tau)
        if key not in cache:
            a, b = views(n, f)
            cache[key] = pm.run(lib, a, b, tau, positive, g=G_UP)
        return cache[key]
    get.lib, get.lib1 = lib, lib1
    return get


def views(n, f, seed=None):
    rng = np.random.RandomState(5000 + 7 * n + f if seed is None else seed)
    a = rng.standard_normal((n, f)).astype(np.float32)
    b = (0.3 * a + rng.standard_normal((n, f))).astype(np.float32)
    return a, b


def bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).tobytes()


def where(got, want):
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return " (in the sign of a zero or in a NaN)"
    i = tuple(bad[0])
    return f": {len(bad)} elements differ, first at {i}: {got[i]!r} != {want[i]!r}"


def forward_z(ops, a, b, tau, positive):
    """Z and Zc of the forward export, [2, N] (its third result, which ops keeps for the backward call)."""
    return ops._info_nce_pair_forward(a, b, float(tau), ops.INFONCE_POSITIVE[positive])[2]


def rows_against_the_mirror(rows, m, positive, tau):
    """The neighbour rule on both lists; returns the largest |row - the mirror's row|."""
    rows = rows.cpu().numpy()
    c = 1.0 if positive == "raw" else 1.0 / tau
    u = c * m["sii"].astype(np.float64) - 1.0 / tau
    for l in range(2):
        L = np.log(m["z"][l])
        allowed = np.stack([u - np.nextafter(L, -np.inf), u - L, u - np.nextafter(L, np.inf)])
        assert (rows[l][None, :] == allowed).any(axis=0).all(), f"a row of list {l} is not c s_ii - 1/tau - log of the mirror's sum"
    return np.abs(rows - m["rows"]).max()


@pytest.mark.parametrize("n,f,positive,tau", CASES)
def test_forward_against_the_mirror(ops, mirror, n, f, positive, tau):
    a, b = views(n, f)
    m = mirror(n, f, positive, tau)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    loss, rows = ops.info_nce_pair(ta, tb, tau=tau, positive=positive, return_rows=True)
    st = dict(ops.last_stats)
    assert (st["rows"], st["features"], st["host_syncs"]) == (n, f, 0)
    assert (st["parts"], st["groups"]) == (mirror.lib.pair_parts(n), mirror.lib.pair_groups(n))
    assert loss.dtype == torch.float64 and loss.dim() == 0 and rows.shape == (2, n)
    z = forward_z(ops, ta, tb, tau, positive).cpu().numpy()
    assert bits(z[0]) == bits(m["z"][0]), "Z" + where(z[0], m["z"][0])
    assert bits(z[1]) == bits(m["z"][1]), "Zc" + where(z[1], m["z"][1])
    err = rows_against_the_mirror(rows, m, positive, tau)
    print(f"n={n} F={f} {positive} tau={tau}: rows max |diff| {err:.3g}, loss diff {abs(float(loss) - m['loss']):.3g}")
    assert err <= 1e-13
    assert abs(float(loss) - m["loss"]) <= 1e-13


@pytest.mark.parametrize("n,f,positive,tau", CASES)
def test_gradients_bit_for_bit_and_against_two_calls(ops, mirror, n, f, positive, tau):
    a, b = views(n, f)
    m = mirror(n, f, positive, tau)
    ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    up = torch.tensor(G_UP, dtype=torch.float64, device="cuda")
    loss = ops.info_nce_pair(ta, tb, tau=tau, positive=positive)
    loss.backward(up)
    assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["rows"] == n
    assert ta.grad.dtype == torch.float32 and ta.grad.shape == (n, f)
    assert bits(ta.grad) == bits(m["ga"]), "ga" + where(ta.grad.cpu().numpy(), m["ga"])
    assert bits(tb.grad) == bits(m["gb"]), "gb" + where(tb.grad.cpu().numpy(), m["gb"])
    # the two-call path on the device
    ua, ub = ta.detach().clone().requires_grad_(True), tb.detach().clone().requires_grad_(True)
    two = 0.5 * (ops.info_nce(ua, ub, tau=tau, positive=positive) + ops.info_nce(ub, ua, tau=tau, positive=positive))
    two.backward(up)
    gmax = max(float(ua.grad.abs().max()), float(ub.grad.abs().max()))
    dl = abs(float(loss.detach()) - float(two.detach()))
    dg = max(float((ta.grad.double() - ua.grad.double()).abs().max()), float((tb.grad.double() - ub.grad.double()).abs().max()))
    print(f"n={n} F={f} {positive} tau={tau}: pair - two calls: loss {dl:.3g} (bound {pair_loss_abs(n):.3g}), gradients {dg / gmax if gmax else 0.0:.3g} of the largest")
    assert dl <= pair_loss_abs(n)
    assert dg <= PAIR_GRAD_BOUND * gmax


def exact_views(n, f):
    """a_i = e_(i mod F), b_j = four entries +-1 in columns drawn per j: powers of two before and after the normalisation."""
    rng = np.random.RandomState(n + f)
    a = np.zeros((n, f), dtype=np.float32)
    a[np.arange(n), np.arange(n) % f] = 1.0
    b = np.zeros((n, f), dtype=np.float32)
    for j in range(n):
        b[j, rng.choice(f, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    return a, b


@pytest.mark.parametrize("n,f", [(65, 8), (300, 40), (129, 33)])
def test_operand_maps_with_exact_data(ops, mirror, n, f):
    """s_ij = bh_j[i mod F], exactly 0 or +-0.5, and S != S^T.  Z_i counts row i of S, Zc_j column j: (count of +0.5) e+ + (count of
    0) e0 + (count of -0.5) e-, exact in float64 in any order; tau = 1/4 spreads the three values by e^2 each, so Z and Zc differ
    widely."""
    tau = 0.25
    a, b = exact_views(n, f)
    s = (b / 2.0)[:, np.arange(n) % f].T                                        # s[i, j] = bh_j[i mod F]
    assert not np.array_equal(s, s.T)
    itf = np.float32(1.0 / tau)
    e = {v: np.float64(im.expw(mirror.lib1, np.array([(np.float32(v) - np.float32(1.0)) * itf], dtype=np.float32))[0]) for v in (-0.5, 0.0, 0.5)}
    z_want = sum((s == v).sum(axis=1) * e[v] for v in (-0.5, 0.0, 0.5))         # over the columns j: Z_i
    zc_want = sum((s == v).sum(axis=0) * e[v] for v in (-0.5, 0.0, 0.5))        # over the rows i: Zc_j
    assert np.median(np.abs(z_want - zc_want) / z_want) > 0.05                  # a swap would show
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    z = forward_z(ops, ta, tb, tau, "raw").cpu().numpy()
    assert bits(z[0]) == bits(z_want), "Z" + where(z[0], z_want)
    assert bits(z[1]) == bits(zc_want), "Zc" + where(z[1], zc_want)
    rows = ops.info_nce_pair(ta, tb, tau=tau, positive="raw", return_rows=True)[1].cpu().numpy()
    want = np.stack([np.diag(s) - 1.0 / tau - np.log(z_want), np.diag(s) - 1.0 / tau - np.log(zc_want)])
    assert np.abs(rows - want).max() <= 1e-13                                   # s_ii exact: diag(s), not a neighbour's
    # the second products: the mirror's bits on the same data (a swap of the reciprocals moves them far: Z != Zc)
    m = pm.run(mirror.lib, a, b, tau, "raw", g=1.0)
    ta.requires_grad_(True)
    tb.requires_grad_(True)
    ops.info_nce_pair(ta, tb, tau=tau, positive="raw").backward()
    assert bits(ta.grad) == bits(m["ga"]) and bits(tb.grad) == bits(m["gb"])
    # and the float64 restatement, which knows nothing of the mirror's operand maps
    loss, ga, gb = pm.restatement(a, b, tau, "raw")
    gmax = max(np.abs(ga).max(), np.abs(gb).max())
    assert max(np.abs(m["ga"] - ga).max(), np.abs(m["gb"] - gb).max()) <= 4 * 1.68e-6 * gmax


def test_two_calls_and_a_poisoned_arena_give_the_same_bits(ops):
    a, b = (torch.from_numpy(x).cuda() for x in views(300, 100))

    def call():
        ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        loss, rows = ops.info_nce_pair(ta, tb, tau=0.4, positive="raw", return_rows=True)
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
    """The check of tests/test_gpu_infonce.py's test_memory_is_linear_in_n -- arena_bytes < n n 4 / 8, an eighth of the similarity
    matrix -- for both pair calls.  The forward passes it at that test's shape, (4096, 64).  The backward call keeps the
    one-direction call's part accumulators (num_parts(N) x Np x Fp floats for each input: 8 parts at 4096 rows, 16.8 MB against the
    8.4 MB of the inequality, as rlap_infonce_backward itself), so both are held to the inequality at (16384, 64), where the parts
    are 2, and to growing no faster than N between the two sizes."""
    f, seen = 64, {}
    for n in (4096, 16384):
        a, b = (torch.from_numpy(x).cuda().requires_grad_(True) for x in views(n, f))
        loss = ops.info_nce_pair(a, b)
        fwd = ops.last_stats["arena_bytes"]
        assert ops.last_stats["host_syncs"] == 0 and math.isfinite(float(loss.detach()))
        loss.backward()
        bwd = ops.last_stats["arena_bytes"]
        assert ops.last_stats["host_syncs"] == 0
        seen[n] = (fwd, bwd)
        assert fwd < n * n * 4 // 8
        if n == 16384:
            assert bwd < n * n * 4 // 8
    assert seen[16384][0] <= 4 * seen[4096][0] + 4096 and seen[16384][1] <= 4 * seen[4096][1] + 4096


def test_zero_rows_and_the_ends_of_tau(ops, mirror):
    a, b = views(70, 9, seed=3)
    a[5] = 0.0
    b[40] = 0.0
    for tau in (1.0 / 32.0, 1024.0):
        m = pm.run(mirror.lib, a, b, tau, "scaled", g=1.0)
        ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
        loss = ops.info_nce_pair(ta, tb, tau=tau)
        loss.backward()
        assert abs(float(loss.detach()) - m["loss"]) <= 1e-13 and bits(ta.grad) == bits(m["ga"]) and bits(tb.grad) == bits(m["gb"])
        assert bool(torch.isfinite(ta.grad).all()) and bool(torch.isfinite(tb.grad).all())


def test_value_errors_come_before_the_device(ops):
    x = torch.zeros(4, 3, device="cuda")
    for bad in ((x.double(), x.double(), 0.4), (x, x[:3], 0.4), (x, x, 0.0), (torch.zeros(2, 513), torch.zeros(2, 513), 0.4)):
        with pytest.raises(ValueError):
            ops.info_nce_pair(bad[0], bad[1], tau=bad[2])


def test_node_contrast_pair_on_snapshot_gcn_conv(ops):
    """The public path of the node-level step with pair=True: two views of BA(300, 3), one GCN layer for both, the loss down to the
    layer's weight; repeated bit for bit; and within the bounds of the default module.  The weight's gradient is a linear map of the
    gradient of h with non-negative coefficients |x|^T A^T (A: the normalised snapshots), so a difference of at most eps gmax in every
    entry of the latter moves an entry of the former by at most eps times that map applied to gmax everywhere -- which one more
    backward pass through the layer on |x| computes."""
    from rlap_amd.adapters import Graph, NodeContrast, SnapshotGCNConv, rLapViews
    n, cin, cout = 300, 16, 32
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((n, cin)).astype(np.float32)).cuda()

    def step(pair):
        torch.manual_seed(3)
        conv = SnapshotGCNConv(cin, cout).cuda()
        snaps = rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2).snapshots(g)
        h = conv(x, snaps)
        h.retain_grad()
        contrast = NodeContrast(tau=0.4, pair=pair)
        loss = contrast(h)
        if pair:
            assert bits(loss) == bits(contrast(h[0], h[1]))
        loss.backward()
        out = (loss.detach(), conv.weight.grad.clone(), conv.bias.grad.clone(), h.grad.clone())
        conv.weight.grad = None
        conv.bias.grad = None
        gmax = float(h.grad.abs().max())
        conv(x.abs(), snaps).backward(torch.full_like(h, gmax))
        return out + (conv.weight.grad.clone(), conv.bias.grad.clone())
    l1, w1, b1, h1, _, _ = step(True)
    l2, w2, b2, h2, _, _ = step(True)
    assert l1.dtype == torch.float64 and math.isfinite(float(l1)) and float(l1) > 0
    assert bool(torch.isfinite(w1).all()) and float(w1.abs().max()) > 0 and bool(torch.isfinite(b1).all())
    assert bits(l1) == bits(l2) and bits(w1) == bits(w2) and bits(b1) == bits(b2)
    l0, w0, b0, h0, w_amp, b_amp = step(False)
    gmax = float(h0.abs().max())
    print(f"pair - default: loss {abs(float(l1) - float(l0)):.3g}, dh {float((h1 - h0).abs().max()) / gmax:.3g} of the largest, "
          f"dw {float(((w1 - w0).abs() / w_amp).max()):.3g} and db {float(((b1 - b0).abs() / b_amp).max()):.3g} of the amplified largest")
    assert abs(float(l1) - float(l0)) <= pair_loss_abs(n)
    assert float((h1 - h0).abs().max()) <= PAIR_GRAD_BOUND * gmax
    assert bool(((w1 - w0).abs() <= PAIR_GRAD_BOUND * w_amp).all()) and bool(((b1 - b0).abs() <= PAIR_GRAD_BOUND * b_amp).all())
