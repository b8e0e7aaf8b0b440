"""Per-graph readout of batched node embeddings on the device (ops.graph_readout, rlap_graph_readout / _backward), its gradient and
the adapters of the graph-level step built on it (rLapViews.snapshots(node_ptr=), Snapshots.aggregate / .readout, SnapshotGINConv).

1. The yardstick is independent of the code under test: torch on the CPU in float64, zeros(G, F).index_add_(0, batch, x[l]).  Per
   element |y - ref| <= 2 n_g u A, u = 2^-53, n_g the nodes of the graph, A = sum |x| over them.  Derived, not measured: a sum of
   n_g terms carries (n_g - 1) u on each side, whatever its order.  The mean adds one rounding, a float32 result one more (2^-24).
   An empty graph gets exactly 0.
2. Bit for bit: the float64 result equals the host mirror (tests/csrc/spmm_mirror.cc around rlap_amd/csrc/rlap_spmm.h, the header the
   kernels include): every element through spmm_entries on the list (node i -> graph g, 1.0), a sample of them through
   spmm_mirror.list_sum(lib, ones, column), the readout's definition.  The float32 result equals the float64 result of the same
   features rounded once.  Twice the same call, per-layer calls, a call on one graph's slice and a poisoned arena give the same bits.
3. last_stats pins the call to its kernels: no host synchronisation, the exact chunk counts of the table.
4. The gradient is the gather, bit for bit; torch.autograd.gradcheck on a table with an empty graph.
5. End to end: two views of a batch of 8 BA(64, 3) graphs through two SnapshotGINConv layers and the readout, against the same
   stack on every graph alone, and repeated.

The shapes are the smallest at which the kernels can go wrong: empty graphs, both sides of a chunk edge (255, 256, 257 nodes),
several chunks (512, 513, 1000), one graph for all ids, 300 small graphs (more chunks than a wave takes at once); F on both sides
of the 16-byte lanes (1, 3), of the staged rows (16, 64 in float32: 4 and 16 lanes a row) and of one wave a row (65, 200).
"""
import numpy as np
import pytest
import torch

import spmm_mirror

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ALL_F = (1, 3, 16, 64, 65, 200)
FMAX = max(ALL_F)
LAYERS = 3
SIZES_A = [0, 1, 255, 256, 257, 0, 512, 513, 1000, 3]


def table_of(sizes):
    return [0] + np.cumsum(sizes).tolist()


TABLES = {
    "chunk_edges": table_of(SIZES_A),
    "one_graph": [0, sum(SIZES_A)],
    "small_graphs": table_of(np.random.RandomState(3).randint(1, 41, size=300).tolist()),
}
NMAX = max(t[-1] for t in TABLES.values())


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return spmm_mirror.build(tmp_path_factory.mktemp("spmm"))


@pytest.fixture(scope="module")
def features():
    """(LAYERS, NMAX, FMAX) float64: mixed signs, magnitudes over ten decades, so that the order of a sum shows in its bits."""
    rng = np.random.RandomState(11)
    x = rng.choice([-1.0, 1.0], size=(LAYERS, NMAX, FMAX)) * 10.0 ** rng.uniform(-5.0, 5.0, size=(LAYERS, NMAX, FMAX))
    return torch.from_numpy(x)


def batch_of(node_ptr):
    p = torch.as_tensor(node_ptr)
    return torch.repeat_interleave(torch.arange(p.numel() - 1), p[1:] - p[:-1])


@pytest.fixture(scope="module")
def yardsticks(features, mirror):
    """Per table and per input precision, computed once at FMAX columns (a column's sum does not depend on the others) and left
    unchanged: ref and A (LAYERS, G, FMAX) by torch on the CPU, and the mirror's bits."""
    out = {}
    for name, node_ptr in TABLES.items():
        N, G = node_ptr[-1], len(node_ptr) - 1
        batch = batch_of(node_ptr)
        for prec in ("f64", "f32"):
            x = features[:, :N]
            if prec == "f32":
                x = x.float().double()
            ref = torch.stack([torch.zeros(G, FMAX, dtype=torch.float64).index_add_(0, batch, x[l]) for l in range(LAYERS)])
            mass = torch.stack([torch.zeros(G, FMAX, dtype=torch.float64).index_add_(0, batch, x[l].abs()) for l in range(LAYERS)])
            M = max(N, G)
            pad = np.zeros((M, FMAX))
            bits = []
            for l in range(LAYERS):
                pad[:N] = x[l].numpy()
                bits.append(spmm_mirror.entries(mirror, np.arange(N), batch.numpy(), np.ones(N), M, pad, False, False)[:G].copy())
            out[name, prec] = {"ref": ref, "mass": mass, "mirror": torch.from_numpy(np.stack(bits))}
    return out


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


def counts_of(node_ptr):
    p = torch.as_tensor(node_ptr)
    return (p[1:] - p[:-1]).double()


def check_stats(ops, node_ptr):
    st = ops.last_stats
    sizes = np.diff(node_ptr)
    assert st["host_syncs"] == 0
    assert st["rows"] == node_ptr[-1] and st["graphs"] == len(node_ptr) - 1
    assert st["chunks"] == int(((sizes + 255) // 256).sum())
    assert st["chunked_graphs"] == int((sizes > 256).sum())
    assert (st["chunked_graphs"] > 0) == bool((sizes > 256).any())
    assert st["arena_bytes"] > 0                      # the export ran: nothing here is computed by torch


@pytest.mark.parametrize("F", ALL_F)
@pytest.mark.parametrize("name", list(TABLES))
def test_against_torch_and_the_mirror(ops, features, yardsticks, mirror, name, F):
    node_ptr = TABLES[name]
    N, G = node_ptr[-1], len(node_ptr) - 1
    n = counts_of(node_ptr)[None, :, None]
    x64 = features[:, :N, :F].contiguous().cuda()
    x32 = x64.float()
    for L in (1, LAYERS):
        for reduce in ("sum", "mean"):
            div = n.clamp_min(1.0) if reduce == "mean" else torch.ones_like(n)
            # float64 against the yardstick and the mirror
            y = ops.graph_readout(x64[:L], node_ptr, reduce=reduce)
            check_stats(ops, node_ptr)
            assert y.shape == (L, G, F) and y.dtype == torch.float64 and y.is_cuda
            ys = yardsticks[name, "f64"]
            ref, mass, bits = ys["ref"][:L, :, :F] / div, ys["mass"][:L, :, :F] / div, ys["mirror"][:L, :, :F] / div
            err, bound = (y.cpu() - ref).abs(), 2 * n * U * mass + (U * ref.abs() if reduce == "mean" else 0)
            print(f"{name} F={F} L={L} {reduce} f64: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3g}")
            assert bool((err <= bound).all())
            assert same_bits(y, bits)
            empty = (n[0, :, 0] == 0)
            assert same_bits(y[:, empty.cuda()], torch.zeros(L, int(empty.sum()), F, dtype=torch.float64))   # exactly +0
            # float32: the float64 result of the same features rounded once
            y32 = ops.graph_readout(x32[:L], node_ptr, reduce=reduce)
            check_stats(ops, node_ptr)
            assert y32.dtype == torch.float32
            assert same_bits(y32, ops.graph_readout(x32[:L].double(), node_ptr, reduce=reduce).float())
            ys = yardsticks[name, "f32"]
            ref, mass = ys["ref"][:L, :, :F] / div, ys["mass"][:L, :, :F] / div
            assert same_bits(y32, (ys["mirror"][:L, :, :F] / div).float())
            bound = 2 * n * U * mass + (U * ref.abs() if reduce == "mean" else 0)
            bound = bound + 2.0 ** -24 * (ref.abs() + bound)
            assert bool(((y32.cpu().double() - ref).abs() <= bound).all())
    # (2-D features are one layer)
    assert same_bits(ops.graph_readout(x64[1], node_ptr), ops.graph_readout(x64[1:2], node_ptr)[0])


def test_the_definition_element_by_element(ops, features, mirror):
    """spmm_mirror.list_sum(lib, ones, column) is the readout's definition: a sample of elements of every graph of the chunk-edge
    table, both precisions of the input."""
    node_ptr = TABLES["chunk_edges"]
    N = node_ptr[-1]
    cols = [0, 2, 64, FMAX - 1]
    x = features[:, :N, :].contiguous()
    y = ops.graph_readout(x.cuda(), node_ptr).cpu()
    ym = ops.graph_readout(x.cuda(), node_ptr, reduce="mean").cpu()
    for g in range(len(node_ptr) - 1):
        s, e = node_ptr[g], node_ptr[g + 1]
        for l in (0, LAYERS - 1):
            for f in cols:
                column = x[l, s:e, f].numpy()
                want = spmm_mirror.list_sum(mirror, np.ones(e - s), column)
                assert np.float64(y[l, g, f].item()).tobytes() == np.float64(want).tobytes(), (g, l, f)
                want_mean = want / np.float64(e - s) if e > s else np.float64(0.0)
                assert np.float64(ym[l, g, f].item()).tobytes() == np.float64(want_mean).tobytes(), (g, l, f)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("F", (1, 16, 64, 200))
@pytest.mark.parametrize("name", list(TABLES))
def test_same_bits_however_it_is_called(ops, features, name, F, dtype):
    node_ptr = TABLES[name]
    N, G = node_ptr[-1], len(node_ptr) - 1
    x = features[:, :N, :F].to(dtype).contiguous().cuda()
    for reduce in ("sum", "mean"):
        y = ops.graph_readout(x, node_ptr, reduce=reduce)
        assert same_bits(y, ops.graph_readout(x, node_ptr, reduce=reduce))                                  # twice
        assert same_bits(y, torch.stack([ops.graph_readout(x[l], node_ptr, reduce=reduce) for l in range(LAYERS)]))   # layer by layer
        graphs = range(G) if G <= 10 else (0, 1, 57, 150, G - 1)
        for g in graphs:                                                                                   # a graph alone
            s, e = node_ptr[g], node_ptr[g + 1]
            alone = ops.graph_readout(x[:, s:e], [0, e - s], reduce=reduce)
            assert same_bits(alone[:, 0], y[:, g]), (g, e - s)
        ops.debug_set_poison(0xA5)
        try:
            assert same_bits(y, ops.graph_readout(x, node_ptr, reduce=reduce))                              # whatever the arena and y held
            xg = x.clone().requires_grad_(True)                                                             # the gather, whatever gx held
            assert same_bits(torch.autograd.grad(ops.graph_readout(xg, node_ptr).sum(), xg)[0], torch.ones_like(x))
        finally:
            ops.debug_set_poison(-1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("F", (1, 3, 64, 200))
@pytest.mark.parametrize("name", list(TABLES))
def test_backward_is_the_gather(ops, features, name, F, dtype):
    node_ptr = TABLES[name]
    N, G = node_ptr[-1], len(node_ptr) - 1
    batch, n = batch_of(node_ptr), counts_of(node_ptr)
    gy = features[:, :G, :F].to(dtype).contiguous().cuda()          # (any values serve as the gradient of y)
    for L in (1, LAYERS):
        for reduce in ("sum", "mean"):
            x = features[:L, :N, :F].to(dtype).contiguous().cuda().requires_grad_(True)
            y = ops.graph_readout(x, node_ptr, reduce=reduce)
            y.backward(gy[:L])
            assert ops.last_stats["host_syncs"] == 0 and ops.last_stats["rows"] == N
            want = gy[:L].cpu()[:, batch]
            if reduce == "mean":
                want = (want.double() / n[batch][None, :, None]).to(dtype)      # one float64 division, rounded once
            assert same_bits(x.grad, want)
    x2 = features[0, :N, :F].to(dtype).contiguous().cuda().requires_grad_(True)   # (num_nodes, F)
    ops.graph_readout(x2, node_ptr).backward(gy[0])
    assert same_bits(x2.grad, gy[0].cpu()[batch])


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_gradcheck(ops, reduce):
    x = torch.from_numpy(np.random.RandomState(5).uniform(-1, 1, size=(2, 5, 3))).cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: ops.graph_readout(t, [0, 2, 2, 5], reduce=reduce), (x,))


# ------------------------------------------------------------------------------------------------ end to end
GRAPHS, NODES, IN, HID = 8, 64, 8, 16


@pytest.fixture(scope="module")
def batch_input():
    from rlap_amd import graphs
    eis = [graphs.barabasi_albert(NODES, 3, 20 + g) + NODES * g for g in range(GRAPHS)]
    x = torch.from_numpy(np.random.RandomState(9).uniform(-1, 1, size=(GRAPHS * NODES, IN))).float()
    return x.cuda(), torch.cat(eis, dim=1).cuda(), [NODES * g for g in range(GRAPHS + 1)]


def gin_stack(identity):
    from rlap_amd import adapters
    torch.manual_seed(4)
    mk = (lambda i, o: torch.nn.Identity()) if identity else (lambda i, o: torch.nn.Linear(i, o))
    return torch.nn.ModuleList([adapters.SnapshotGINConv(mk(IN, HID), eps=0.25, train_eps=True),
                                adapters.SnapshotGINConv(mk(HID, HID), eps=0.0, train_eps=True)]).cuda()


def embed(convs, x, holder):
    """The graph-level encoder of scripts/graph_shared.py in small: GIN layers, a readout after each, concatenated."""
    z, outs = x, []
    for conv in convs:
        z = torch.relu(conv(z, holder))
        outs.append(holder.readout(z))
    return torch.cat(outs, dim=-1), z


@pytest.mark.parametrize("identity", [True, False])
def test_views_gin_readout_end_to_end(ops, batch_input, identity):
    from rlap_amd import adapters
    x, edge_index, node_ptr = batch_input
    aug = adapters.rLapViews(fracs=(0.25, 0.5), o_v="random", o_n="asc", keep_weights=True, seed=12)
    holder = aug.snapshots((x, edge_index, None), node_ptr=node_ptr)
    assert holder.layers == 2 and holder.node_ptr.tolist() == node_ptr
    assert aug.num_remove == [[int(0.25 * NODES)] * GRAPHS, [int(0.5 * NODES)] * GRAPHS]
    convs = gin_stack(identity)
    with torch.no_grad():
        emb, z = embed(convs, x, holder)
    assert emb.shape == (2, GRAPHS, (IN if identity else HID) * 2)
    ptr = holder.ptr.tolist()
    for k in range(2):
        for g in range(GRAPHS):          # (view k, graph g) alone: its rows, its ids from 0
            part = holder.sc[ptr[k * GRAPHS + g]:ptr[k * GRAPHS + g + 1]].clone()
            part[:, :2] -= node_ptr[g]
            alone = adapters.Snapshots(part, [0, int(part.shape[0])], NODES, None, True, 1.0)
            with torch.no_grad():
                e1, z1 = embed(convs, x[node_ptr[g]:node_ptr[g + 1]], alone)
            if identity:
                assert same_bits(e1[0, 0], emb[k, g]), (k, g)
            else:
                # the dense products of the two runs have other shapes and may round differently: the float32 bound of check 1 on
                # the pooled embeddings, 2 n_g 2^-24 A with A the sum of |z| over the graph (the last layer's for both halves
                # would be too small for the first: each half has its own)
                with torch.no_grad():
                    zs, a = x[node_ptr[g]:node_ptr[g + 1]], []
                    for conv in convs:
                        zs = torch.relu(conv(zs, alone))
                        a.append(zs[0].abs().double().sum(0))
                bound = 2 * NODES * 2.0 ** -24 * torch.cat(a)
                assert bool(((e1[0, 0].double() - emb[k, g].double()).abs() <= bound).all()), (k, g)

    def step(h):
        xs = x.clone().requires_grad_(True)
        for p in convs.parameters():
            p.grad = None
        e, _ = embed(convs, xs, h)
        (e * torch.linspace(-1, 1, e.numel(), device=e.device).reshape(e.shape)).sum().backward()
        return e.detach(), [xs.grad.clone()] + [p.grad.clone() for p in convs.parameters()]

    e1, g1 = step(holder)
    assert same_bits(e1, emb)
    assert all(t.abs().sum() > 0 for t in g1) and len(g1) == 1 + len(list(convs.parameters()))   # x, eps and the weights are reached
    e2, g2 = step(holder)
    assert same_bits(e1, e2) and all(same_bits(a, b) for a, b in zip(g1, g2))
    planned = holder.plan()
    e3, g3 = step(planned)
    e4, g4 = step(planned)
    assert planned.aggregate_plan is not None and planned.snapshot_plan is None          # GIN needs the second plan alone
    assert same_bits(e3, e1) and same_bits(e3, e4)
    assert all(same_bits(a, b) for a, b in zip(g3, g4)) and all(same_bits(a, b) for a, b in zip(g3, g1))
