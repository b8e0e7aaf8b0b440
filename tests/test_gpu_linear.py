"""The fused dense layer on the device (ops.linear_act, rlap_linear_act / rlap_linear_act_backward) against its host
mirror (tests/csrc/linear_mirror.cc around rlap_amd/csrc/rlap_linear.h, the header the kernels include).

Shapes: M in {1, 31, 32, 33, 127, 128, 129} and 2112 (at 512 -> 512 the weight gradient has 64 parts of its 66 row tiles: more than
one part, fewer parts than tiles), Fin and Fout in {1, 2, 3, 31, 32, 33, 64, 65, 128, 129, 257, 512}, every value on each side, the
corners (1, 512), (512, 1), (512, 512).  What reaches what:

  k_lin_product<1, 1>  output width <= 32;  <2, 1>  33, 64;  <4, 1>  65, 128;  <4, 2>  129 (5 tiles, the second of wave 0 alone);
                       <4, 3>  257 (9 tiles, the third of wave 0 alone);  <4, 4>  512.  The forward takes the instance of Fout,
                       the input gradient that of Fin: every width stands on each side, so either mode sees every instance.
  k_lin_cross<1>       Fout <= 64;  <2>  65, 128;  <4>  129, 257, 512; clamped tiles at 65, 129, 257 on either side
  lane paths           widths divisible by 4 take 16-byte loads, the others 4-byte ones; one case moves x off the 16-byte grid

y, gx, gW and gb equal the mirror's bits under none and relu.  Under elu every element is within one float32 unit in the last
place: the device's float64 expm1 may differ from glibc's in the last place of a double, which moves the float32 rounding by at
most one step; every other operation is IEEE.  The backward mirror reads the DEVICE's y, as the device's backward does.  The mirror
runs once per case (a module-wide cache) and serves every test.
"""
import numpy as np
import pytest
import torch

import linear_mirror as lm
from util import ba_graph

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 512), (31, 512, 1), (2112, 512, 512), (32, 2, 3), (33, 3, 2), (127, 31, 33), (128, 32, 64), (129, 33, 31), (33, 64, 32),
          (129, 65, 128), (127, 128, 65), (31, 129, 257), (32, 257, 129)]
# every shape under none or relu (equal bits), every other one under elu too; the bias and the weight's layout cycle
CASES = [(m, fin, fout, ("relu", "none")[k % 2], 1.0, k % 3 != 2, k % 2 == 1) for k, (m, fin, fout) in enumerate(SHAPES)] + \
        [(m, fin, fout, "elu", (1.0, 0.5)[(k // 2) % 2], True, k % 4 == 0) for k, (m, fin, fout) in enumerate(SHAPES) if k % 2 == 0]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return lm.build(tmp_path_factory.mktemp("linear"))


def case_inputs(m, fin, fout, bias, out_in, cache={}):
    key = (m, fin, fout, bias, out_in)
    if key not in cache:
        x, w, b, gy = lm.inputs(m, fin, fout, 7000 + 13 * m + 5 * fin + fout, bias)
        cache[key] = (x, np.ascontiguousarray(w.T) if out_in else w, b, gy)
    return cache[key]


def dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


def host(t):
    return t.detach().cpu().numpy()


def ulps(got, want):
    """The largest distance of two float32 arrays in units in the last place (0 for equal bits; NaNs must match)."""
    a, b = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b))
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia, ib = np.where(ia < 0, -(ia & 0x7FFFFFFF), ia), np.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    d = np.where(np.isnan(a), 0, np.abs(ia - ib))
    return int(d.max()) if d.size else 0


def run(ops, x, w, b, gy, act, alpha, out_in):
    """One forward and backward through autograd: y and the three gradients, on the host."""
    tx, tw = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
    tb = None if b is None else dev(b).requires_grad_(True)
    y = ops.linear_act(tx, tw, tb, act=act, alpha=alpha, weight_layout="out_in" if out_in else "in_out")
    stats = dict(ops.last_stats)
    y.backward(dev(gy))
    return host(y), host(tx.grad), host(tw.grad), None if tb is None else host(tb.grad), stats


@pytest.mark.parametrize("m,fin,fout,act,alpha,bias,out_in", CASES)
def test_the_device_against_the_mirror(ops, mirror, m, fin, fout, act, alpha, bias, out_in):
    x, w, b, gy = case_inputs(m, fin, fout, bias, out_in)
    y, gx, gw, gb, stats = run(ops, x, w, b, gy, act, alpha, out_in)
    want_y = lm.forward(mirror, x, w, b, act, alpha, out_in)
    want = lm.backward(mirror, x, w, y, gy, act, alpha, out_in)                 # from the device's y
    worst = {"y": ulps(y, want_y), "gx": ulps(gx, want["gx"]), "gw": ulps(gw, want["gw"]), "gb": 0 if gb is None else ulps(gb, want["gb"])}
    print(f"m={m} {fin}->{fout} {act} bias={bias} out_in={out_in}: ulps {worst}, parts {stats['parts']}")
    assert max(worst.values()) <= (1 if act == "elu" else 0), worst
    assert stats["rows"] == m and stats["fin"] == fin and stats["fout"] == fout and stats["host_syncs"] == 0
    if act != "none" and m * fout >= 100:
        assert (y > 0).any() and ((y <= 0).any())
    assert gw.shape == w.shape and y.shape == (m, fout)


def test_more_than_one_part_and_fewer_parts_than_tiles(ops, mirror):
    assert mirror.lin_num_parts(2112, 512, 512) == 64 and (2112 + 31) // 32 == 66
    assert mirror.lin_num_parts(129, 65, 128) == 5 and mirror.lin_num_parts(32, 257, 129) == 1


@pytest.mark.parametrize("act", ["none", "elu"])
def test_x_off_the_16_byte_grid_takes_the_other_lane_path_and_gives_the_same_bits(ops, mirror, act):
    m, fin, fout = 129, 64, 32
    x, w, b, gy = case_inputs(m, fin, fout, True, False)
    big = torch.empty(m * fin + 1, dtype=torch.float32, device="cuda")
    off = big[1:].view(m, fin)
    off.copy_(dev(x))
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    outs = []
    for tx in (dev(x), off):
        tx = tx.detach().requires_grad_(True)
        tw = dev(w).requires_grad_(True)
        y = ops.linear_act(tx, tw, dev(b), act=act)
        y.backward(dev(gy))
        outs.append((host(y), host(tx.grad), host(tw.grad)))
    for a, o in zip(*outs):
        assert a.tobytes() == o.tobytes()
    assert ulps(outs[0][0], lm.forward(mirror, x, w, b, act)) <= (1 if act == "elu" else 0)
    assert outs[0][2].tobytes() == lm.backward(mirror, x, w, outs[0][0], gy, act, want=("gw",))["gw"].tobytes()


def test_two_calls_give_equal_bits(ops):
    x, w, b, gy = case_inputs(129, 65, 128, True, False)
    a, c = run(ops, x, w, b, gy, "elu", 1.0, False), run(ops, x, w, b, gy, "elu", 1.0, False)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a[:4], c[:4]))


@pytest.mark.parametrize("act", ["relu", "elu"])
def test_a_layered_call_is_its_layers_and_its_flattened_rows(ops, act):
    L, n, fin, fout = 3, 45, 33, 20
    x, w, b, gy = lm.inputs(L * n, fin, fout, 77)
    y3, gx3, gw3, gb3, stats = run(ops, x.reshape(L, n, fin), w, b, gy.reshape(L, n, fout), act, 1.0, False)
    assert y3.shape == (L, n, fout) and gx3.shape == (L, n, fin) and stats["rows"] == L * n
    for l in range(L):
        yl, gxl, _, _, _ = run(ops, x.reshape(L, n, fin)[l], w, b, gy.reshape(L, n, fout)[l], act, 1.0, False)
        assert yl.tobytes() == y3[l].tobytes() and gxl.tobytes() == gx3[l].tobytes()
    y2, gx2, gw2, gb2, _ = run(ops, x, w, b, gy, act, 1.0, False)
    assert y2.tobytes() == y3.tobytes() and gx2.tobytes() == gx3.tobytes() and gw2.tobytes() == gw3.tobytes() and gb2.tobytes() == gb3.tobytes()


def test_only_the_required_gradients_are_computed(ops, mirror):
    x, w, b, gy = case_inputs(127, 31, 33, True, False)
    full = run(ops, x, w, b, gy, "relu", 1.0, False)
    tw = dev(w).requires_grad_(True)
    y = ops.linear_act(dev(x), tw, dev(b), act="relu")                        # the first layer of a network: no gx, no gb
    y.backward(dev(gy))
    assert host(tw.grad).tobytes() == full[2].tobytes()
    tx = dev(x).requires_grad_(True)
    ops.linear_act(tx, dev(w), None, act="relu").backward(dev(gy))
    nb = lm.forward(mirror, x, w, None, "relu")
    assert host(tx.grad).tobytes() == lm.backward(mirror, x, w, nb, gy, "relu", want=("gx",))["gx"].tobytes()


# ------------------------------------------------------------------------------------------------ the adapters
def test_mlp_and_projection_head_are_the_composition_of_calls(ops):
    from rlap_amd.adapters import ProjectionHead, SnapshotMLP
    x, _, _, _ = lm.inputs(2 * 70, 33, 1, 3)
    for mod, act in ((SnapshotMLP(33, 40, 20), "relu"), (ProjectionHead(33, 12), "elu")):
        torch.manual_seed(11)
        mod = mod.cuda()
        tx = dev(x).reshape(2, 70, 33).requires_grad_(True)
        out = mod(tx)
        gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).cuda()
        out.backward(gy)
        ux = dev(x).reshape(2, 70, 33).requires_grad_(True)
        ws = [p.detach().clone().requires_grad_(True) for p in (mod.fc1.weight, mod.fc1.bias, mod.fc2.weight, mod.fc2.bias)]
        want = ops.linear_act(ops.linear_act(ux, ws[0], ws[1], act=act, weight_layout="out_in"), ws[2], ws[3], weight_layout="out_in")
        want.backward(gy)
        assert torch.equal(out, want) and torch.equal(tx.grad, ux.grad)
        for p, q in zip((mod.fc1.weight, mod.fc1.bias, mod.fc2.weight, mod.fc2.bias), ws):
            assert torch.equal(p.grad, q.grad)
        ref = torch.nn.functional.linear(getattr(torch.nn.functional, act)(torch.nn.functional.linear(ux.detach().double(), ws[0].detach().double(), ws[1].detach().double())),
                                         ws[2].detach().double(), ws[3].detach().double())
        assert float((out.detach().double() - ref).abs().max()) <= 1e-4 * float(ref.abs().max())


def test_gcn_conv_with_the_device_product(ops):
    from rlap_amd.adapters import Graph, SnapshotGCNConv, rLapViews
    n, cin, cout = 300, 16, 33
    g = Graph(None, torch.from_numpy(ba_graph(n, 3, 5)).cuda(), None)
    x = torch.from_numpy(np.random.RandomState(1).standard_normal((n, cin)).astype(np.float32)).cuda()
    snaps = rLapViews((0.25, 0.4), "random", "asc", keep_weights=True, seed=2).snapshots(g)
    torch.manual_seed(3)
    conv = SnapshotGCNConv(cin, cout, dense="device").cuda()
    torch.manual_seed(3)
    old = SnapshotGCNConv(cin, cout).cuda()
    assert torch.equal(conv.weight, old.weight)
    with torch.no_grad():
        conv.bias.add_(0.5)
        old.bias.add_(0.5)
    h = conv(x, snaps)
    assert torch.equal(h, snaps.propagate(ops.linear_act(x, conv.weight)) + conv.bias)
    h.sum().backward()
    assert bool(torch.isfinite(conv.weight.grad).all()) and float(conv.weight.grad.abs().max()) > 0
    assert torch.equal(old(x, snaps), snaps.propagate(x @ old.weight) + old.bias)        # dense="torch" is what it was
    assert float((h - old(x, snaps)).detach().abs().max()) <= 1e-4 * float(h.detach().abs().max())


def test_gin_encoder_with_the_device_product_follows_the_torch_one(ops):
    """SnapshotGINEncoder(dense="device") with the default encoder's parameters: the same embeddings up to the float32 products'
    rounding; the default encoder itself is torch's modules, as before."""
    from rlap_amd import graphs
    from rlap_amd.adapters import SnapshotGINEncoder, rLapViews
    nodes, cin, hid = [40, 45, 35], 7, 32
    node_ptr = [0] + list(np.cumsum(nodes))
    eis = [graphs.barabasi_albert(ng, 2, 30 + k) + node_ptr[k] for k, ng in enumerate(nodes)]
    x = torch.from_numpy(np.random.RandomState(2).standard_normal((node_ptr[-1], cin)).astype(np.float32)).cuda()
    snaps = rLapViews(fracs=(0.2, 0.4), o_v="random", o_n="asc", keep_weights=False, seed=5).snapshots(
        (x, torch.cat(eis, dim=1).cuda(), None), node_ptr=node_ptr)
    torch.manual_seed(4)
    old = SnapshotGINEncoder(cin, hid, 2).cuda()
    new = SnapshotGINEncoder(cin, hid, 2, dense="device").cuda()
    for a, b in zip(new.layers, old.layers):
        a.nn.fc1.load_state_dict(b.nn[0].state_dict())
        a.nn.fc2.load_state_dict(b.nn[2].state_dict())
    z0, g0 = old(x, snaps)
    z1, g1 = new(x, snaps)
    assert z1.shape == z0.shape and g1.shape == g0.shape
    assert float((z1 - z0).detach().abs().max()) <= 1e-3 * float(z0.detach().abs().max())
    z1.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in new.parameters())
