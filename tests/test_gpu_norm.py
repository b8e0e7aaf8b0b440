"""The per-view batch norm with fused activations on the device (ops.batch_norm, adapters.SnapshotBatchNorm, adapters.SnapshotGINEncoder;
DESIGN 4.25) against its host mirror (tests/csrc/norm_mirror.cc around rlap_amd/csrc/rlap_norm.h), bit for bit:

1. A sparse cross product of N in {2, 3, 255, 256, 257, 513} (the edges of the chunk and the minimum), F in {1, 3, 4, 31, 32, 33, 64,
   65, 100, 256, 516} (the edges of the lane paths; 516 is more than two 256-column tiles) and L in {1, 3}, the flags cycling through
   pre x post x slope form x affine x mode: y, stat, the updated running buffers, gx, gweight, gbias and gslope equal the mirror's
   bits, and the info struct reports the path the case means to test (16 bytes a lane iff F % 4 == 0).
2. A view whose storage starts one float off the 16-byte grid at F = 64 takes the scalar path, its aligned twin the vector path;
   both give the same bits.
3. A case sized from the launchers' constants (the mirror exports them) so that every strided launch takes a second round: the
   smallest such shape at F = 4 is L = MAX_GRID * GROUP_WAVES + 1 layers of two rows.
4. A NaN planted in one column stays in its column.
5. Autograd: layer l of an (L, N, F) call equals the (N, F) call on it alone; two runs give equal bits.
6. End to end: SnapshotGINEncoder on a batch of 3 small graphs, two views, through a plan.
"""
import numpy as np
import pytest
import torch

import norm_mirror as nm

pytestmark = pytest.mark.gpu

NS = [2, 3, 255, 256, 257, 513]
FS = [1, 3, 4, 31, 32, 33, 64, 65, 100, 256, 516]
COMBOS = [("none", "none", False, True), ("relu", "none", False, True), ("relu", "relu", False, False), ("none", "prelu", False, True),
          ("relu", "prelu", True, True), ("none", "relu", False, True), ("relu", "prelu", False, False), ("none", "prelu", True, False)]
CASES = []
for i, f in enumerate(FS):
    for j in (0, 3):
        k = 2 * i + (j > 0)
        CASES.append((3 if (i + j) % 2 else 1, NS[(i + j) % 6], f) + COMBOS[k % 8] + (k % 5 != 4,))


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return nm.build(tmp_path_factory.mktemp("norm"))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


def same_bits(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def cuda(a, grad=False):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda().requires_grad_(grad)


def arguments(d, f, pre, post, per_channel, affine, training):
    slope = None if post != "prelu" else (d["slope"] if per_channel else d["slope"][:1])
    return {"weight": d["weight"] if affine else None, "bias": d["bias"] if affine else None, "slope": slope,
            "running_mean": d["running_mean"], "running_var": d["running_var"]}, nm.flags_of(pre, post, per_channel and post == "prelu" and f > 1, training)


def device_run(ops, x, gy, kw, pre, post, training, vec):
    """ops.batch_norm forward and backward on the device: (y, stat, buffers, gradients), the path asserted on the way."""
    tx = x if isinstance(x, torch.Tensor) else cuda(x)
    tx = tx.detach().requires_grad_(True)
    t = {k: cuda(v, k in ("weight", "bias", "slope")) for k, v in kw.items()}
    flags = nm.flags_of(pre, post, kw["slope"] is not None and len(kw["slope"]) > 1, training)
    rm, rv = t["running_mean"].clone(), t["running_var"].clone()
    _, stat, _ = ops._norm_forward(tx.detach(), t["weight"], t["bias"], t["slope"], rm, rv, 0.1, 1e-5, flags)
    assert ops.last_stats["vec"] == int(vec) and ops.last_stats["host_syncs"] == 0
    assert ops.last_stats["launches"] == (3 if training else 1)
    y = ops.batch_norm(tx, t["weight"], t["bias"], t["running_mean"], t["running_var"], training=training, pre=pre, post=post, slope=t["slope"])
    assert same_bits(rm, t["running_mean"]) and same_bits(rv, t["running_var"])
    y.backward(gy if isinstance(gy, torch.Tensor) else cuda(gy))
    assert ops.last_stats["vec"] == int(vec) and ops.last_stats["host_syncs"] == 0
    grads = {"gx": tx.grad, "gweight": None if t["weight"] is None else t["weight"].grad, "gbias": None if t["bias"] is None else t["bias"].grad,
             "gslope": None if t["slope"] is None else t["slope"].grad}
    return y, stat, (t["running_mean"], t["running_var"]), grads


def against_the_mirror(mirror, d, kw, flags, training, y, stat, bufs, grads):
    m = nm.forward(mirror, d["x"], flags=flags, **kw)
    assert same_bits(y, m["y"])
    if training:
        assert same_bits(stat, m["stat"])
        assert same_bits(bufs[0], m["running_mean"]) and same_bits(bufs[1], m["running_var"])
        assert not same_bits(bufs[0], d["running_mean"])
    else:
        assert stat is None and same_bits(bufs[0], d["running_mean"]) and same_bits(bufs[1], d["running_var"])
    b = nm.backward(mirror, d["x"], d["gy"], m["stat"], flags=flags, **{k: v for k, v in kw.items()})
    assert same_bits(grads["gx"], b["gx"])
    for key in ("gweight", "gbias", "gslope"):
        if grads[key] is not None:
            assert same_bits(grads[key], b[key]), key


@pytest.mark.parametrize("L,n,f,pre,post,per_channel,affine,training", CASES)
def test_bits_equal_the_mirror(mirror, ops, L, n, f, pre, post, per_channel, affine, training):
    d = nm.inputs(L, n, f, 1000 + 7 * n + f)
    kw, flags = arguments(d, f, pre, post, per_channel, affine, training)
    y, stat, bufs, grads = device_run(ops, d["x"], d["gy"], kw, pre, post, training, vec=f % 4 == 0)
    against_the_mirror(mirror, d, kw, flags, training, y, stat, bufs, grads)


def test_a_view_off_the_16_byte_grid_takes_the_scalar_path(mirror, ops):
    L, n, f = 2, 257, 64
    d = nm.inputs(L, n, f, 5)
    kw, flags = arguments(d, f, "relu", "prelu", True, True, True)
    base = torch.zeros(L * n * f + 1, dtype=torch.float32, device="cuda")
    base[1:] = cuda(d["x"]).reshape(-1)
    off = base[1:].view(L, n, f)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    out_off = device_run(ops, off, d["gy"], kw, "relu", "prelu", True, vec=False)
    out_on = device_run(ops, d["x"], d["gy"], kw, "relu", "prelu", True, vec=True)
    against_the_mirror(mirror, d, kw, flags, True, *out_off)
    against_the_mirror(mirror, d, kw, flags, True, *out_on)


def test_every_strided_launch_takes_a_second_round(mirror, ops):
    c = nm.constants(mirror)
    L, n, f = c["max_grid"] * c["group_waves"] + 1, 2, 4
    assert mirror.norm_num_items(L, n, f, 1) == L and mirror.norm_num_items(L - 1, n, f, 1) == c["max_grid"] * c["group_waves"]
    d = nm.inputs(L, n, f, 11)
    kw, flags = arguments(d, f, "relu", "prelu", False, True, True)
    out = device_run(ops, d["x"], d["gy"], kw, "relu", "prelu", True, vec=True)
    against_the_mirror(mirror, d, kw, flags, True, *out)


def test_a_nan_stays_in_its_column(mirror, ops):
    """Without activations, so that the NaN is not compared away (v > 0 is false for it): the column's y, gx, statistics and weight
    gradient are NaN as the mirror's are, and no other column changes a bit."""
    L, n, f = 1, 257, 8
    d = nm.inputs(L, n, f, 13)
    kw, flags = arguments(d, f, "none", "none", False, True, True)
    clean = device_run(ops, d["x"], d["gy"], kw, "none", "none", True, vec=True)
    d["x"][0, 100, 5] = np.nan
    y, stat, bufs, grads = device_run(ops, d["x"], d["gy"], kw, "none", "none", True, vec=True)
    m = nm.forward(mirror, d["x"], flags=flags, **kw)
    b = nm.backward(mirror, d["x"], d["gy"], m["stat"], flags=flags, **kw)
    others = [k for k in range(f) if k != 5]
    for got, want, ref in ((y, m["y"], clean[0]), (grads["gx"], b["gx"], clean[3]["gx"])):
        got = got.detach().cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[0, :, 5]).all()
        assert same_bits(got[..., others], ref.detach().cpu().numpy()[..., others])
    for got, want, ref in ((grads["gweight"], b["gweight"], clean[3]["gweight"]), (grads["gbias"], b["gbias"], clean[3]["gbias"]),
                           (bufs[0], m["running_mean"], clean[2][0]), (bufs[1], m["running_var"], clean[2][1])):
        got = got.detach().cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True) and same_bits(got[others], ref.detach().cpu().numpy()[others])
    assert np.isnan(grads["gweight"].cpu().numpy()[5]) and np.isnan(bufs[0].cpu().numpy()[5]) and np.isnan(bufs[1].cpu().numpy()[5])


def test_a_layer_equals_the_call_on_it_alone_and_runs_repeat(ops):
    L, n, f = 3, 513, 33
    d = nm.inputs(L, n, f, 17)
    kw, _ = arguments(d, f, "relu", "prelu", True, True, True)
    kw["running_mean"] = kw["running_var"] = None
    t = {k: cuda(v) for k, v in kw.items()}

    def run(x, gy):
        tx = cuda(x, True)
        w, b, s = (t[k].clone().requires_grad_(True) for k in ("weight", "bias", "slope"))
        y = ops.batch_norm(tx, w, b, pre="relu", post="prelu", slope=s)
        y.backward(cuda(gy))
        return y, tx.grad, w.grad, b.grad, s.grad

    one = run(d["x"], d["gy"])
    two = run(d["x"], d["gy"])
    assert all(same_bits(a, b) for a, b in zip(one, two))
    for l in range(L):
        y, gx = run(d["x"][l], d["gy"][l])[:2]
        assert y.shape == (n, f) and same_bits(y, one[0][l]) and same_bits(gx, one[1][l])


# ------------------------------------------------------------------------------------------------ end to end
GRAPH_NODES, IN, HID, LAYERS = [12, 15, 13], 5, 8, 2


def test_gin_encoder_end_to_end(mirror, ops):
    from rlap_amd import adapters, graphs
    node_ptr = [0] + list(np.cumsum(GRAPH_NODES))
    eis = [graphs.barabasi_albert(ng, 2, 30 + g) + node_ptr[g] for g, ng in enumerate(GRAPH_NODES)]
    n = node_ptr[-1]
    x = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, size=(n, IN))).float().cuda()
    aug = adapters.rLapViews(fracs=(0.2, 0.4), o_v="random", o_n="asc", keep_weights=False, seed=5)
    holder = aug.snapshots((x, torch.cat(eis, dim=1).cuda(), None), node_ptr=node_ptr)
    planned = holder.plan()
    torch.manual_seed(6)
    enc = adapters.SnapshotGINEncoder(IN, HID, LAYERS).cuda()
    seen = []
    hooks = [conv.register_forward_hook(lambda mod, args, out: seen.append((args[0].detach().cpu(), out.detach().cpu()))) for conv in enc.layers]

    def step():
        for p in enc.parameters():
            p.grad = None
        for bn in enc.batch_norms:
            bn.reset_parameters()
        z, g = enc(x, planned)
        up = lambda t: torch.linspace(-1, 1, t.numel(), device=t.device).reshape(t.shape)
        ((z * up(z)).sum() + (g * up(g)).sum()).backward()
        return [z.detach(), g.detach()] + [p.grad.clone() for p in enc.parameters()] + [b.clone() for bn in enc.batch_norms for b in bn.buffers()]

    one = step()
    first = list(seen)
    two = step()
    for h in hooks:
        h.remove()
    assert one[0].shape == (2, n, HID * LAYERS) and one[1].shape == (2, len(GRAPH_NODES), HID * LAYERS)
    assert all(same_bits(a, b) for a, b in zip(one, two))
    assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in enc.parameters())
    assert all(int(bn.num_batches_tracked) == 2 for bn in enc.batch_norms) and planned.aggregate_plan is not None

    # the float64 restatement on the CPU, layer by layer on what the layer was given: the neighbour sum by index_add_, the MLP, then
    # one batch norm call per view, in order.  The conv is float32 on the device: every output is a neighbour sum and two dense
    # products, at most max degree + IN + HID + 4 float32 operations deep, each within 2^-24 of the magnitudes it adds.
    ptr, sc, G = holder.ptr.tolist(), holder.sc.cpu(), len(GRAPH_NODES)
    for i, ((zin, zout), conv, bn) in enumerate(zip(first, enc.layers, enc.batch_norms)):
        lin1, lin2 = conv.nn[0], conv.nn[2]
        w1, b1, w2, b2 = (p.detach().cpu().double() for p in (lin1.weight, lin1.bias, lin2.weight, lin2.bias))
        for k in range(2):
            rows = sc[ptr[k * G]:ptr[(k + 1) * G]]
            zk = (zin if zin.dim() == 2 else zin[k]).double()
            agg, mag = torch.zeros_like(zk), torch.zeros_like(zk)
            agg.index_add_(0, rows[:, 0].long(), zk[rows[:, 1].long()])
            mag.index_add_(0, rows[:, 0].long(), zk[rows[:, 1].long()].abs())
            want = torch.relu((zk + agg) @ w1.T + b1) @ w2.T + b2
            size = (((zk.abs() + mag) @ w1.abs().T + b1.abs()) @ w2.abs().T + b2.abs())
            deg = int(torch.bincount(rows[:, 0].long(), minlength=n).max())
            assert bool(((zout[k].double() - want).abs() <= (deg + IN + HID + 4) * 2.0 ** -24 * size).all()), (i, k)
        rm, rv = nm.torch_buffers(zout.numpy(), np.zeros(HID, dtype=np.float32), np.ones(HID, dtype=np.float32), 0.1, 1e-5, "relu")
        got_m, got_v = bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy()
        assert (np.abs(got_m - rm) <= np.spacing(np.abs(rm))).all() and (np.abs(got_v - rv) <= np.spacing(np.abs(rv))).all(), i
        m = nm.forward(mirror, zout.numpy(), weight=np.ones(HID, dtype=np.float32), bias=np.zeros(HID, dtype=np.float32),
                       running_mean=np.zeros(HID, dtype=np.float32), running_var=np.ones(HID, dtype=np.float32), flags=nm.PRE_RELU)
        assert same_bits(one[0][..., i * HID:(i + 1) * HID].contiguous(), m["y"]) and same_bits(got_m, m["running_mean"])
