"""The fused graph-to-local losses on the device (ops.g2l_jsd / ops.g2l_bootstrap, rlap_g2l_*) against their host mirror
(tests/csrc/g2l_mirror.cc around rlap_amd/csrc/rlap_g2l.h, the header the kernels include).

Shapes: N at the edges of the 32-node tiles and of the workgroup's 128-node block (1, 31, 32, 33, 65, 300), G on both paths -- one
graph with the corrupted embeddings (the vector kernels), and 2, 31, 33, 65 graphs (the matrix-core kernels: one to three graph
tiles, padding graphs in the last one) --, F at the edges of the MFMA's k pair, of the 8-column fragment group, of the 16-byte loads
and of the 32-column feature tiles of the backward accumulators (1, 3, 32, 33, 100, 256, 512 -- 1, 2, 4, 8 and 16 tiles: every
template instance of both backward kernels, each completely filled; 256, 128 and 32 rows a block of the single-graph vector
kernels, and 64 as well for the bootstrap's), in a sparse cross product.  The other tile counts, the single-graph kernels at 64 rows
a block, both sides of each edge of the rows a block, and part counts below the tile count (every case here has one part per node
tile) are tests/test_gpu_loss_regimes.py's.  Tables: "even" (graph boundaries inside 32-node tiles), "empty" (empty graphs at the
front, in the middle and at the end), "one" (one graph holds every node, the others are empty).  The mirror runs once per shape (a
module-wide cache) and serves every test.

  JSD        dh, dneg, dg equal the mirror's bit for bit.  The loss, and pos_i and neg_i element by element
             (test_jsd_rows_against_the_mirror), agree within 1e-13 relative to the mirror's value: the device's float64 log1p may
             differ from the host's in the last place and nothing else may.  The rule takes log1p(e) - ln 2 in one piece,
             log1p((e - 1) / 2), so that this last place is relative to the term however small the term comes out.  Measured on an
             MI355X over these cases: loss at most 5.72e-16, pos_i 2.20e-16, neg_i 1.20e-14 (one row of (N, G, F) = (300, 33, 1),
             whose 32 terms cancel; every other case at most 3.52e-16).  The tests print every figure before they assert.
  bootstrap  c_i, dh and the loss equal the mirror's bit for bit.
"""
import math

import numpy as np
import pytest
import torch

import g2l_mirror as gm
from util import ba_graph

pytestmark = pytest.mark.gpu

# (N, G, F, table)
CASES = [
    (1, 1, 1, None), (31, 1, 3, None), (32, 1, 32, None), (33, 1, 33, None), (65, 1, 100, None), (300, 1, 512, None), (300, 1, 1, None),
    (1, 2, 1, "even"), (31, 2, 3, "even"), (32, 31, 32, "empty"), (33, 33, 33, "one"), (65, 65, 100, "empty"), (300, 2, 512, "even"),
    (300, 33, 1, "even"), (65, 31, 512, "one"), (300, 65, 33, "empty"), (65, 33, 256, "even"),
]
G_UP = 0.75
REL = 1e-13


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


def inputs(n, G, f):
    rng = np.random.RandomState(7000 + 13 * n + 5 * G + f)
    h = (0.5 * rng.standard_normal((n, f))).astype(np.float32)
    g = rng.standard_normal((G, f)).astype(np.float32)
    neg = (0.5 * rng.standard_normal((n, f))).astype(np.float32) if G == 1 else None
    return h, g, neg


def table_of(n, G, kind):
    return None if kind is None else gm.table(n, G, kind)


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    lib = gm.build(tmp_path_factory.mktemp("g2l"))
    cache = {}

    def get(which, n, G, f, kind):
        key = (which, n, G, f, kind)
        if key not in cache:
            h, g, neg = inputs(n, G, f)
            t = table_of(n, G, kind)
            cache[key] = gm.run_jsd(lib, h, g, t, neg, gup=G_UP) if which == "jsd" else gm.run_bootstrap(lib, h, g, t, gup=G_UP)
        return cache[key]
    get.lib = lib
    return get


def bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).tobytes()


def same(got, want, what):
    got = got.detach().cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.asarray(got))
    want = torch.from_numpy(np.ascontiguousarray(want))
    if torch.equal(got, want):
        return
    bad = (got != want).nonzero()
    i = tuple(bad[0].tolist()) if len(bad) else None
    raise AssertionError(f"{what}: {len(bad)} elements differ" + (f", first at {i}: {got[i]!r} != {want[i]!r}" if i is not None else " (NaN)"))


def close(got, want):
    """The largest |got - want| / |want| (0 where both are 0)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    diff = np.abs(got - want)
    return float(np.where(diff == 0, 0.0, diff / np.maximum(np.abs(want), 1e-300)).max()) if got.size else 0.0


def cuda(x):
    return torch.from_numpy(x).cuda() if x is not None else None


@pytest.mark.parametrize("n,G,f,kind", CASES)
def test_jsd_against_the_mirror(ops, mirror, n, G, f, kind):
    h, g, neg = inputs(n, G, f)
    t = table_of(n, G, kind)
    m = mirror("jsd", n, G, f, kind)
    th, tg = cuda(h).requires_grad_(True), cuda(g).requires_grad_(True)
    tn = cuda(neg).requires_grad_(True) if neg is not None else None
    loss, rows = ops.g2l_jsd(th, tg, node_ptr=t, neg=tn, return_rows=True)
    st = dict(ops.last_stats)
    assert (st["rows"], st["graphs"], st["features"], st["host_syncs"]) == (n, G, f, 0)
    assert st["parts"] == mirror.lib.g2l_parts(n, G, f) and st["arena_bytes"] == mirror.lib.g2l_arena_bytes(gm.JSD_FORWARD, n, G, f)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and rows.shape == (2, n) and rows.dtype == torch.float64
    el = close(float(loss.detach()), m["loss"])
    print(f"jsd n={n} G={G} F={f}: loss rel {el:.3g}")
    assert el <= REL
    loss.backward(torch.tensor(G_UP, dtype=torch.float64, device=loss.device))
    st = dict(ops.last_stats)
    assert st["host_syncs"] == 0 and st["arena_bytes"] == mirror.lib.g2l_arena_bytes(gm.JSD_BACKWARD, n, G, f)
    assert th.grad.dtype == torch.float32 and th.grad.shape == (n, f) and tg.grad.shape == (G, f)
    same(th.grad, m["gh"], "dh")
    same(tg.grad, m["gg"], "dg")
    if tn is not None:
        same(tn.grad, m["gneg"], "dneg")


@pytest.mark.parametrize("n,G,f,kind", CASES)
def test_jsd_rows_against_the_mirror(ops, mirror, n, G, f, kind):
    """pos_i and neg_i within 1e-13 relative to the mirror's, element by element."""
    h, g, neg = inputs(n, G, f)
    m = mirror("jsd", n, G, f, kind)
    rows = ops.g2l_jsd(cuda(h), cuda(g), node_ptr=table_of(n, G, kind), neg=cuda(neg), return_rows=True)[1].cpu().numpy()
    ep, en = close(rows[0], m["pos"]), close(rows[1], m["neg"])
    print(f"jsd rows n={n} G={G} F={f}: pos rel {ep:.3g}, neg rel {en:.3g}; largest |diff| pos {np.abs(rows[0] - m['pos']).max():.3g}, "
          f"neg {np.abs(rows[1] - m['neg']).max():.3g}")
    assert ep <= REL and en <= REL


@pytest.mark.parametrize("n,G,f,kind", CASES)
def test_bootstrap_against_the_mirror(ops, mirror, n, G, f, kind):
    h, g, _ = inputs(n, G, f)
    t = table_of(n, G, kind)
    m = mirror("bootstrap", n, G, f, kind)
    th = cuda(h).requires_grad_(True)
    loss, rows = ops.g2l_bootstrap(th, cuda(g), node_ptr=t, return_rows=True)
    st = dict(ops.last_stats)
    assert (st["rows"], st["graphs"], st["features"], st["host_syncs"]) == (n, G, f, 0)
    assert st["arena_bytes"] == mirror.lib.g2l_arena_bytes(gm.BOOT_FORWARD, n, G, f)
    assert loss.dtype == torch.float64 and loss.dim() == 0 and rows.shape == (n,)
    same(rows, m["c"], "c")
    assert bits(loss) == bits(np.float64(m["loss"])), (float(loss.detach()), m["loss"])
    loss.backward(torch.tensor(G_UP, dtype=torch.float64, device=loss.device))
    assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["arena_bytes"] == mirror.lib.g2l_arena_bytes(gm.BOOT_BACKWARD, n, G, f)
    same(th.grad, m["gh"], "dh")


@pytest.mark.parametrize("G", [1, 33])
def test_two_calls_and_a_poisoned_arena_give_the_same_bits(ops, G):
    n, f = 300, 100
    h, g, neg = (cuda(x) for x in inputs(n, G, f))
    t = table_of(n, G, None if G == 1 else "empty")

    def call():
        th, tg = h.clone().requires_grad_(True), g.clone().requires_grad_(True)
        tn = neg.clone().requires_grad_(True) if neg is not None else None
        loss, rows = ops.g2l_jsd(th, tg, node_ptr=t, neg=tn, return_rows=True)
        loss.backward()
        tb = h.clone().requires_grad_(True)
        bl, c = ops.g2l_bootstrap(tb, g, node_ptr=t, return_rows=True)
        bl.backward()
        return [bits(x) for x in (loss, rows, th.grad, tg.grad, bl, c, tb.grad)] + ([bits(tn.grad)] if tn is not None else [])
    base = call()
    assert call() == base
    for byte in (0xFF, 0x00, 0x3C):
        ops.debug_set_poison(byte)
        try:
            assert call() == base, f"poison {byte:#x}"
        finally:
            ops.debug_set_poison(-1)
    assert ops.last_stats["host_syncs"] == 0


def test_exact_scores_pin_the_map_and_the_exclusions(ops, mirror):
    """h_i = e_(i mod F) / 4 and g_j = four entries +-1 per graph: every score is exactly 0 or +-0.25, so neg_i is a count of three
    values and the positive of node i is g(i)'s entry -- a wrong map, a padding graph or the positive inside the sum would show."""
    n, G, f = 130, 37, 8
    rng = np.random.RandomState(3)
    h = np.zeros((n, f), dtype=np.float32)
    h[np.arange(n), np.arange(n) % f] = 0.25
    g = np.zeros((G, f), dtype=np.float32)
    for j in range(G):
        g[j, rng.choice(f, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    t = gm.table(n, G, "empty")
    batch = gm.batch_of(t, n)
    s = h.astype(np.float64) @ g.astype(np.float64).T
    loss, rows = ops.g2l_jsd(cuda(h), cuda(g), node_ptr=t, return_rows=True)
    rows = rows.cpu().numpy()
    pos_of = {v: mirror.lib.g2l_pos_term(v) for v in (-0.25, 0.0, 0.25)}
    neg_of = {v: mirror.lib.g2l_neg_term(v) for v in (-0.25, 0.0, 0.25)}
    want_pos = np.array([pos_of[s[i, batch[i]]] for i in range(n)])
    mask = np.ones((n, G), dtype=bool)
    mask[np.arange(n), batch] = False
    want_neg = sum(((s == v) & mask).sum(axis=1) * neg_of[v] for v in (-0.25, 0.0, 0.25))
    assert close(rows[0], want_pos) <= REL
    assert np.abs(rows[1] - want_neg).max() <= 1e-12        # (a sum of up to 36 terms of size 0.1 in another order)
    m = gm.run_jsd(mirror.lib, h, g, t)
    assert close(rows[1], m["neg"]) <= REL and close(float(loss), m["loss"]) <= REL


def test_a_score_that_is_not_finite_gives_a_nan_loss(ops):
    for G in (1, 3):
        h, g, neg = inputs(40, G, 5)
        h[7, 2] = float("inf")
        loss = ops.g2l_jsd(cuda(h), cuda(g), node_ptr=table_of(40, G, None if G == 1 else "even"), neg=cuda(neg))
        assert math.isnan(float(loss))


def test_value_errors_come_before_the_device(ops):
    x = torch.zeros(4, 3, device="cuda")
    g1, g2 = torch.zeros(1, 3, device="cuda"), torch.zeros(2, 3, device="cuda")
    for bad in (dict(h=x.double(), g=g1.double(), neg=x.double()), dict(h=x, g=g1), dict(h=x, g=g2, node_ptr=[0, 2, 4], neg=x),
                dict(h=x, g=g2), dict(h=torch.zeros(2, 513), g=torch.zeros(1, 513), neg=torch.zeros(2, 513))):
        with pytest.raises(ValueError):
            ops.g2l_jsd(**bad)
    with pytest.raises(ValueError):
        ops.g2l_bootstrap(x, g1.clone().requires_grad_(True))


def test_g2l_contrast_on_snapshot_gcn_conv(ops):
    """The public path of scripts/node_dedicated.py in small: two views of BA(300, 3) from one elimination call, one GCN layer for
    both, the pass on the corrupted input, summaries sigmoid(mean readout) through a linear layer, G2LContrast; loss.backward()
    reaches the layer's weight; the whole step repeats bit for bit."""
    from rlap_amd.adapters import G2LContrast, Graph, SnapshotGCNConv, corrupt, rLapViews
    n, cin, cout = 300, 16, 32
    graph = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((n, cin)).astype(np.float32)).cuda()

    def step():
        torch.manual_seed(3)
        conv = SnapshotGCNConv(cin, cout).cuda()
        project = torch.nn.Linear(cout, cout).cuda()
        snaps = rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2).snapshots(graph)
        h = conv(x, snaps)
        hn = conv(corrupt(x, generator=torch.Generator(device="cuda").manual_seed(8)), snaps)
        assert h.shape == (2, n, cout) and hn.shape == (2, n, cout) and h.dtype == torch.float32
        g = project(torch.sigmoid(ops.graph_readout(h, [0, n], reduce="mean")))
        assert g.shape == (2, 1, cout)
        contrast = G2LContrast()
        loss = contrast(h, g1=g, h3=hn)
        both = contrast(h[0], h[1], g[0], g[1], hn[0], hn[1])
        assert bits(loss) == bits(both)
        loss.backward()
        return loss.detach(), conv.weight.grad.clone(), project.weight.grad.clone()
    l1, w1, p1 = step()
    l2, w2, p2 = step()
    assert l1.dtype == torch.float64 and math.isfinite(float(l1))
    assert bool(torch.isfinite(w1).all()) and float(w1.abs().max()) > 0 and float(p1.abs().max()) > 0
    assert bits(l1) == bits(l2) and bits(w1) == bits(w2) and bits(p1) == bits(p2)


def test_bootstrap_g2l_on_snapshot_gin_conv(ops):
    """The public path of scripts/graph_shared_g2l.py in small: two views of a batch of three small graphs, one GIN layer, a
    predictor on the nodes, the readout as the targets, BootstrapG2L; gradients reach the layer and the predictor; repeats bit for
    bit."""
    from rlap_amd import adapters, graphs
    sizes = [40, 25, 64]
    node_ptr = [0, 40, 65, 129]
    eis = [graphs.barabasi_albert(s, 3, 20 + k) + node_ptr[k] for k, s in enumerate(sizes)]
    x = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, size=(129, 8))).float().cuda()
    edge_index = torch.cat(eis, dim=1).cuda()

    def step():
        torch.manual_seed(4)
        conv = adapters.SnapshotGINConv(torch.nn.Linear(8, 16), eps=0.25, train_eps=True).cuda()
        predictor = torch.nn.Linear(16, 16).cuda()
        holder = adapters.rLapViews(fracs=(0.25, 0.5), o_v="random", o_n="asc", keep_weights=True, seed=12).snapshots((x, edge_index, None), node_ptr=node_ptr)
        z = torch.relu(conv(x, holder))
        assert z.shape == (2, 129, 16)
        targets = holder.readout(z)
        assert targets.shape == (2, 3, 16)
        pred = predictor(z)
        loss = adapters.BootstrapG2L()(pred, g1_target=targets, node_ptr=node_ptr)
        pair = adapters.BootstrapG2L()(pred[0], pred[1], targets[0], targets[1], node_ptr=node_ptr)
        assert bits(loss) == bits(pair)
        loss.backward()
        return loss.detach(), predictor.weight.grad.clone(), conv.nn.weight.grad.clone()
    l1, p1, w1 = step()
    l2, p2, w2 = step()
    assert l1.dtype == torch.float64 and math.isfinite(float(l1)) and abs(float(l1)) <= 129 / 3 + 1e-6
    assert float(p1.abs().max()) > 0 and float(w1.abs().max()) > 0 and bool(torch.isfinite(w1).all())
    assert bits(l1) == bits(l2) and bits(p1) == bits(p2) and bits(w1) == bits(w2)
