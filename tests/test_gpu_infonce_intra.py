"""The InfoNCE calls with intraview negatives on the device (ops.info_nce / ops.info_nce_pair with intraview="masked" | "all",
rlap_infonce_intra and its three kin) against their host mirror (tests/csrc/infonce_intra_mirror.cc around
rlap_amd/csrc/rlap_infonce.h, the header the kernels include).

Shapes, each the smallest that hits its place: N = 1 and 2 (a tile of one and two rows: the diagonal is all or half of the intraview
stream), 31, 32, 33 and 64, 65 (the diagonal in the last lane of a tile, in the first lane of the next, in a tile of one row), 127, 128,
129 (the row block's edge: the diagonal in the last owner tile of a half-empty block), 300 (several parts of one tile), 2708 (a part
holds several tiles and the diagonal tile lies inside one of them).  Every N has two or three F of {1, 3, 32, 33, 100, 256, 512}, and
each of the five ladder instances of the backward kernel (F <= 32, 64, 128, 256, 512) meets an N on each side of a tile edge; F <= 33
at N = 2708 so that the mirror stays within seconds.  Every shape runs both variants, one-way and pair; `positive` and tau go round.
The mirror runs once per case.

  forward    Z (the pair: and Zc) equal the mirror's bit for bit.  Each row term is fl(u - L) with u = c s_ii - 1/tau from the MIRROR's
             s_ii and L one of log(Z) and its two neighbours (the rule of tests/test_gpu_infonce.py), within 1e-13 of the mirror's;
             the loss within 1e-13.
  backward   ga and gb equal the mirror's bit for bit.
  operands   exact data: rows that are signed unit vectors make every similarity 0 or +-1, S^ab is not symmetric, and every Z is a
             count of three values of expw whose float64 sum is exact in any order: a diagonal mask that is misplaced, transposed or
             applied to the wrong stream changes Z by a whole term.
"""
import math

import numpy as np
import pytest
import torch

import infonce_intra_mirror as xm
import infonce_mirror as im
from util import ba_graph

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 33), (2, 3), (2, 100), (31, 3), (31, 256), (32, 32), (32, 512), (33, 33), (33, 100), (64, 1), (64, 256), (65, 32),
          (65, 512), (127, 100), (127, 3), (128, 256), (128, 33), (129, 512), (129, 1), (300, 256), (300, 100), (300, 33), (2708, 33), (2708, 3)]
CASES = [(n, f, ("scaled", "raw")[(k + v + p) % 2], (0.4, 1.0 / 32.0, 2.0)[(k + p) % 3], variant, pair)
         for k, (n, f) in enumerate(SHAPES) for v, variant in enumerate(("masked", "all")) for p, pair in enumerate((False, True))]
G_UP = 0.75


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    lib = xm.build(tmp_path_factory.mktemp("infonce_intra"))
    lib1 = im.build(tmp_path_factory.mktemp("infonce_one"))      # the one-direction mirror: its expw export
    cache = {}

    def get(n, f, positive, tau, variant, pair):
        key = (n, f, positive, tau, variant, pair)
        if key not in cache:
            a, b = views(n, f)
            cache[key] = xm.run(lib, a, b, tau, positive, variant, g=G_UP, pair=pair)
        return cache[key]
    get.lib, get.lib1 = lib, lib1
    return get


def views(n, f, seed=None):
    rng = np.random.RandomState(6000 + 7 * n + f if seed is None else seed)
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


def call(ops, pair):
    return ops.info_nce_pair if pair else ops.info_nce


def forward_z(ops, a, b, tau, positive, variant, pair):
    """The row sums of the forward export ([N]; the pair: [2, N]), its third result, which ops keeps for the backward call."""
    fn = ops._info_nce_pair_forward if pair else ops._info_nce_forward
    return fn(a, b, float(tau), ops.INFONCE_POSITIVE[positive], ops.INFONCE_INTRAVIEW[variant])[2]


def rows_against_the_mirror(rows, m, positive, tau):
    """The neighbour rule on every list; returns the largest |row - the mirror's row|."""
    rows = rows.cpu().numpy()
    c = 1.0 if positive == "raw" else 1.0 / tau
    u = c * m["sii"].astype(np.float64) - 1.0 / tau
    for got, z in zip(np.atleast_2d(rows), np.atleast_2d(m["z"])):
        L = np.log(z)
        allowed = np.stack([u - np.nextafter(L, -np.inf), u - L, u - np.nextafter(L, np.inf)])
        assert (got[None, :] == allowed).any(axis=0).all(), "a row is not c s_ii - 1/tau - log of the mirror's sum"
    return np.abs(rows - m["rows"]).max()


@pytest.mark.parametrize("n,f,positive,tau,variant,pair", CASES)
def test_forward_and_gradients_against_the_mirror(ops, mirror, n, f, positive, tau, variant, pair):
    a, b = views(n, f)
    m = mirror(n, f, positive, tau, variant, pair)
    ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
    loss, rows = call(ops, pair)(ta, tb, tau=tau, positive=positive, return_rows=True, intraview=variant)
    st = dict(ops.last_stats)
    assert (st["rows"], st["features"], st["host_syncs"]) == (n, f, 0)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and rows.shape == ((2, n) if pair else (n,))
    z = forward_z(ops, ta, tb, tau, positive, variant, pair).cpu().numpy()
    assert bits(z) == bits(m["z"]), "Z" + where(z, m["z"])
    err = rows_against_the_mirror(rows, m, positive, tau)
    print(f"n={n} F={f} {positive} tau={tau} {variant} pair={pair}: rows max |diff| {err:.3g}, loss diff {abs(float(loss.detach()) - m['loss']):.3g}")
    assert err <= 1e-13
    assert abs(float(loss.detach()) - m["loss"]) <= 1e-13
    loss.backward(torch.tensor(G_UP, dtype=torch.float64, device="cuda"))
    assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["rows"] == n
    assert ta.grad.dtype == torch.float32 and ta.grad.shape == (n, f)
    assert bits(ta.grad) == bits(m["ga"]), "ga" + where(ta.grad.cpu().numpy(), m["ga"])
    assert bits(tb.grad) == bits(m["gb"]), "gb" + where(tb.grad.cpu().numpy(), m["gb"])


@pytest.mark.parametrize("pair", [False, True])
@pytest.mark.parametrize("variant", ["masked", "all"])
@pytest.mark.parametrize("n,f", [(65, 8), (300, 40), (129, 33)])
def test_operand_maps_with_exact_data(ops, mirror, n, f, variant, pair):
    """s is exactly 0 or +-1 everywhere.  Z_i counts row i of S^ab and row i of S^aa (without column i when masked), Zc_j column j of
    S^ab and row j of S^bb: (count of +1) e+ + (count of 0) e0 + (count of -1) e-, exact in float64 in any order at tau = 1/4."""
    tau = 0.25
    a, b = xm.exact_views(n, f)
    sab, saa, sbb = a @ b.T, a @ a.T, b @ b.T
    assert not np.array_equal(sab, sab.T) and not np.array_equal(saa, sbb)
    itf = np.float32(1.0 / tau)
    e = {v: np.float64(im.expw(mirror.lib1, np.array([(np.float32(v) - np.float32(1.0)) * itf], dtype=np.float32))[0]) for v in (-1.0, 0.0, 1.0)}
    assert e[1.0] == 1.0
    keep = np.ones((n, n)) if variant == "all" else 1.0 - np.eye(n)
    count = lambda s, axis, w: sum(((s == v) * w).sum(axis=axis) * e[v] for v in (-1.0, 0.0, 1.0))
    z_want = count(sab, 1, 1.0) + count(saa, 1, keep)
    zc_want = count(sab, 0, 1.0) + count(sbb, 1, keep)
    assert np.abs(z_want - zc_want).max() > 0.5                                 # a swap of the lists would show
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    z = forward_z(ops, ta, tb, tau, "raw", variant, pair).cpu().numpy()
    want = np.stack([z_want, zc_want]) if pair else z_want
    assert bits(z) == bits(want), "Z" + where(z, want)
    rows = call(ops, pair)(ta, tb, tau=tau, positive="raw", return_rows=True, intraview=variant)[1].cpu().numpy()
    assert np.abs(rows - (np.diag(sab) - 1.0 / tau - np.log(want))).max() <= 1e-13   # the positive is s^ab_ii, exact
    # the second products: the mirror's bits on the same data, and the float64 restatement, which knows nothing of the operand maps
    m = xm.run(mirror.lib, a, b, tau, "raw", variant, g=1.0, pair=pair)
    ta.requires_grad_(True)
    tb.requires_grad_(True)
    call(ops, pair)(ta, tb, tau=tau, positive="raw", intraview=variant).backward()
    assert bits(ta.grad) == bits(m["ga"]) and bits(tb.grad) == bits(m["gb"])
    loss, ga, gb = xm.restatement(a, b, tau, "raw", variant, pair=pair)
    gmax = max(np.abs(ga).max(), np.abs(gb).max())
    assert max(np.abs(m["ga"] - ga).max(), np.abs(m["gb"] - gb).max()) <= 4 * 3.78e-6 * gmax   # tests/test_infonce_intra_cpu.py's bound


@pytest.mark.parametrize("pair", [False, True])
def test_two_calls_and_a_poisoned_arena_give_the_same_bits(ops, pair):
    a, b = (torch.from_numpy(x).cuda() for x in views(300, 100))

    def run(variant):
        ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        loss, rows = call(ops, pair)(ta, tb, tau=0.4, positive="raw", return_rows=True, intraview=variant)
        loss.backward()
        return [bits(t) for t in (loss, rows, ta.grad, tb.grad)]
    for variant in ("masked", "all"):
        base = run(variant)
        assert run(variant) == base
        for byte in (0xFF, 0x00, 0x3C):
            ops.debug_set_poison(byte)
            try:
                assert run(variant) == base, f"poison {byte:#x}"
            finally:
                ops.debug_set_poison(-1)
    assert ops.last_stats["host_syncs"] == 0
    assert run("masked") != run("all") and run("masked") != run("none")


@pytest.mark.parametrize("pair", [False, True])
def test_none_is_the_plain_call_bit_for_bit(ops, pair):
    a, b = (torch.from_numpy(x).cuda() for x in views(129, 33))
    ta, tb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    call(ops, pair)(ta, tb, tau=0.4).backward()
    ua, ub = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    call(ops, pair)(ua, ub, tau=0.4, intraview="none").backward()
    assert bits(ta.grad) == bits(ua.grad) and bits(tb.grad) == bits(ub.grad)


def test_zero_rows_and_the_ends_of_tau(ops, mirror):
    a, b = views(70, 9, seed=3)
    a[5] = 0.0
    b[40] = 0.0
    for tau, variant, pair in ((1.0 / 32.0, "masked", False), (1024.0, "all", True), (1.0 / 32.0, "all", False), (1024.0, "masked", True)):
        m = xm.run(mirror.lib, a, b, tau, "scaled", variant, g=1.0, pair=pair)
        ta, tb = torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda().requires_grad_(True)
        loss = call(ops, pair)(ta, tb, tau=tau, intraview=variant)
        loss.backward()
        assert abs(float(loss.detach()) - m["loss"]) <= 1e-13 and bits(ta.grad) == bits(m["ga"]) and bits(tb.grad) == bits(m["gb"])
        assert bool(torch.isfinite(ta.grad).all()) and bool(torch.isfinite(tb.grad).all())


def test_memory_is_linear_in_n(ops):
    """arena_bytes < n n 4 / 8, an eighth of ONE similarity matrix (the torch path keeps an N x 2N one per direction), at (16384, 64)
    for all four calls, and growing no faster than N from (4096, 64)."""
    f, seen = 64, {}
    for n in (4096, 16384):
        for pair in (False, True):
            a, b = (torch.from_numpy(x).cuda().requires_grad_(True) for x in views(n, f))
            loss = call(ops, pair)(a, b, intraview="masked")
            fwd = ops.last_stats["arena_bytes"]
            assert ops.last_stats["host_syncs"] == 0 and math.isfinite(float(loss.detach()))
            loss.backward()
            bwd = ops.last_stats["arena_bytes"]
            assert ops.last_stats["host_syncs"] == 0
            seen[n, pair] = (fwd, bwd)
            assert fwd < n * n * 4 // 8
            if n == 16384:
                assert bwd < n * n * 4 // 8
    for pair in (False, True):
        assert seen[16384, pair][0] <= 4 * seen[4096, pair][0] + 4096 and seen[16384, pair][1] <= 4 * seen[4096, pair][1] + 4096


def test_value_errors_come_before_the_device(ops):
    x = torch.zeros(4, 3, device="cuda")
    for fn in (ops.info_nce, ops.info_nce_pair):
        for bad in ("both", None, 1, True):
            with pytest.raises(ValueError):
                fn(x, x, intraview=bad)
        with pytest.raises(ValueError):
            fn(x, x[:3], intraview="all")


@pytest.mark.parametrize("pair", [False, True])
def test_node_contrast_with_intraview_negatives_on_snapshot_gcn_conv(ops, pair):
    """The public path of the node-level step with intraview_negs=True: two views of BA(300, 3), one GCN layer for both, the loss down
    to the layer's weight; repeated bit for bit; the loss is the two-view value of ops with intraview="masked" and exceeds the plain
    one (every denominator gained positive terms)."""
    from rlap_amd.adapters import Graph, NodeContrast, SnapshotGCNConv, rLapViews
    n, cin, cout = 300, 16, 32
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((n, cin)).astype(np.float32)).cuda()

    def step(setting):
        torch.manual_seed(3)
        conv = SnapshotGCNConv(cin, cout).cuda()
        snaps = rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2).snapshots(g)
        h = conv(x, snaps)
        loss = NodeContrast(tau=0.4, pair=pair, intraview_negs=setting)(h)
        loss.backward()
        return loss.detach(), conv.weight.grad.clone(), conv.bias.grad.clone(), h.detach()
    l1, w1, b1, h = step(True)
    l2, w2, b2, _ = step(True)
    assert l1.dtype == torch.float64 and math.isfinite(float(l1)) and float(l1) > 0
    assert bool(torch.isfinite(w1).all()) and float(w1.abs().max()) > 0 and bool(torch.isfinite(b1).all())
    assert bits(l1) == bits(l2) and bits(w1) == bits(w2) and bits(b1) == bits(b2)
    if pair:
        assert bits(l1) == bits(ops.info_nce_pair(h[0], h[1], tau=0.4, positive="raw", intraview="masked"))
    else:
        want = 0.5 * (ops.info_nce(h[0], h[1], tau=0.4, positive="raw", intraview="masked") + ops.info_nce(h[1], h[0], tau=0.4, positive="raw", intraview="masked"))
        assert bits(l1) == bits(want)
    l0, w0, _, _ = step(False)
    la, wa, _, _ = step("all")
    assert float(l0) < float(l1) < float(la) and bits(w0) != bits(w1) != bits(wa)
