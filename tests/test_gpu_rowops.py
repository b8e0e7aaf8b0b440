"""The fused bias-activation-dropout pass and the per-row layer norm on the device (ops.bias_act_dropout, ops.layer_norm and the
modules around them) against their host mirror (tests/csrc/rowops_mirror.cc around rlap_amd/csrc/rlap_rowops.h), bit
for bit:

1. A sparse cross product of N in {1, 2, 3, 255, 256, 257, 513} (the edges of the chunk), F in {1, 3, 4, 31, 32, 33, 64, 65, 100,
   128, 129, 256, 516, 1024, 4096} (the edges of the lane paths, of the rows that share a wave and of the row kernel's instances)
   and L in {1, 3}, the flags cycling through the activations, both slope forms, with and without parameters, p in {0, 0.2}: y, gx,
   gbias, gweight and gslope of both calls equal the mirror's bits, and the info struct reports the path (16 bytes a lane iff
   F % 4 == 0) and the instance the case means to test.
2. A view whose storage starts one float off the 16-byte grid takes the scalar path, its aligned twin the vector path; both give
   the same bits, dropout mask included.
3. L = MAX_GRID * GROUP_WAVES + 1 layers of two rows at F = 4 (sized from the launchers' constants): every strided launch takes a
   second round.
4. A planted NaN stays in its row (layer norm) or its element (epilogue); two runs give equal bits; layer l of a call equals the
   call on x[l] with seed + l; the backward pass draws the forward's mask again (gx == 0 exactly where y was dropped).
5. End to end: SnapshotG2LEncoder with both norm choices on three graphs of 40 nodes, two views, through a plan, and
   SnapshotGCNConv(epilogue=...).
"""
import numpy as np
import pytest
import torch

import rowops_mirror as rm

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 255, 256, 257, 513]
FS = [1, 3, 4, 31, 32, 33, 64, 65, 100, 128, 129, 256, 516, 1024, 4096]
COMBOS = [("none", False, True), ("relu", False, True), ("prelu", False, True), ("prelu", True, True), ("relu", False, False),
          ("prelu", True, False), ("none", False, False), ("prelu", False, False)]
CASES = []
for i, f in enumerate(FS):
    for j in (0, 4):
        k = 2 * i + (j > 0)
        n = NS[(i + j) % 7]
        if f >= 1024:
            n = min(n, 257)       # (the mirror's time: a few million elements a case at the most)
        CASES.append((3 if (i + j) % 2 else 1, n, f) + COMBOS[k % 8] + (0.2 if k % 3 else 0.0,))
assert 25 <= len(CASES) <= 30
INSTANCE = {f: (1 if f <= 256 else 2 if f <= 512 else 4 if f <= 1024 else 8 if f <= 2048 else 16) for f in FS}


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return rm.build(tmp_path_factory.mktemp("rowops"))


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


def arguments(d, f, act, per_channel, params):
    slope = None if act != "prelu" else (d["slope"] if per_channel and f > 1 else d["slope"][:1])
    return {"weight": d["weight"] if params else None, "bias": d["bias"] if params else None, "slope": slope}, rm.flags_of(act, per_channel and f > 1 and act == "prelu", True)


def device_epilogue(ops, x, gy, kw, act, p, seed, vec):
    """ops.bias_act_dropout forward and backward on the device: (y, gradients), the path asserted on the way."""
    tx = (x if isinstance(x, torch.Tensor) else cuda(x)).detach().requires_grad_(True)
    b, s = cuda(kw["bias"], True), cuda(kw["slope"], True)
    y = ops.bias_act_dropout(tx, b, act=act, slope=s, p=p, seed=seed)
    assert (ops.last_stats["vec"], ops.last_stats["launches"], ops.last_stats["host_syncs"], ops.last_stats["arena_bytes"]) == (int(vec), 1, 0, 0)
    y.backward(gy if isinstance(gy, torch.Tensor) else cuda(gy))
    assert ops.last_stats["vec"] == int(vec) and ops.last_stats["host_syncs"] == 0
    assert ops.last_stats["launches"] == (3 if b is not None or s is not None else 1)
    return y, {"gx": tx.grad, "gbias": None if b is None else b.grad, "gslope": None if s is None else s.grad}


def device_layer_norm(ops, x, gy, kw, post, p, seed, vec, instance):
    tx = (x if isinstance(x, torch.Tensor) else cuda(x)).detach().requires_grad_(True)
    w, b, s = cuda(kw["weight"], True), cuda(kw["bias"], True), cuda(kw["slope"], True)
    y = ops.layer_norm(tx, w, b, post=post, slope=s, p=p, seed=seed)
    assert (ops.last_stats["vec"], ops.last_stats["launches"], ops.last_stats["instance"], ops.last_stats["host_syncs"]) == (int(vec), 1, instance, 0)
    y.backward(gy if isinstance(gy, torch.Tensor) else cuda(gy))
    assert (ops.last_stats["vec"], ops.last_stats["instance"], ops.last_stats["host_syncs"]) == (int(vec), instance, 0)
    assert ops.last_stats["launches"] == (4 if w is not None or s is not None else 1)
    return y, {"gx": tx.grad, "gweight": None if w is None else w.grad, "gbias": None if b is None else b.grad, "gslope": None if s is None else s.grad}


def epilogue_against_the_mirror(mirror, d, kw, flags, p, seed, y, grads):
    assert same_bits(y, rm.forward(mirror, d["x"], kw["bias"], kw["slope"], p, seed, flags))
    m = rm.backward(mirror, d["x"], d["gy"], kw["bias"], kw["slope"], p, seed, flags)
    for key in ("gx", "gbias", "gslope"):
        if grads[key] is not None:
            assert same_bits(grads[key], m[key]), key


def layer_norm_against_the_mirror(mirror, d, kw, flags, p, seed, y, grads):
    assert same_bits(y, rm.ln_forward(mirror, d["x"], kw["weight"], kw["bias"], kw["slope"], 1e-5, p, seed, flags)[0])
    m = rm.ln_backward(mirror, d["x"], d["gy"], kw["weight"], kw["bias"], kw["slope"], 1e-5, p, seed, flags)
    for key in ("gx", "gweight", "gbias", "gslope"):
        if grads[key] is not None:
            assert same_bits(grads[key], m[key]), key


@pytest.mark.parametrize("L,n,f,act,per_channel,params,p", CASES)
def test_bits_equal_the_mirror(mirror, ops, L, n, f, act, per_channel, params, p):
    d = rm.inputs(L, n, f, 1000 + 7 * n + f)
    kw, flags = arguments(d, f, act, per_channel, params)
    seed = 31 * n + f
    y, grads = device_epilogue(ops, d["x"], d["gy"], kw, act, p, seed, vec=f % 4 == 0)
    epilogue_against_the_mirror(mirror, d, kw, flags, p, seed, y, grads)
    y, grads = device_layer_norm(ops, d["x"], d["gy"], kw, act, p, seed, vec=f % 4 == 0, instance=INSTANCE[f])
    layer_norm_against_the_mirror(mirror, d, kw, flags, p, seed, y, grads)


@pytest.mark.parametrize("f", [64, 516])
def test_a_view_off_the_16_byte_grid_takes_the_scalar_path(mirror, ops, f):
    L, n = 2, 257
    d = rm.inputs(L, n, f, 5)
    kw, flags = arguments(d, f, "prelu", True, True)
    base = torch.zeros(L * n * f + 1, dtype=torch.float32, device="cuda")
    base[1:] = cuda(d["x"]).reshape(-1)
    off = base[1:].view(L, n, f)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    epilogue_against_the_mirror(mirror, d, kw, flags, 0.2, 9, *device_epilogue(ops, off, d["gy"], kw, "prelu", 0.2, 9, vec=False))
    epilogue_against_the_mirror(mirror, d, kw, flags, 0.2, 9, *device_epilogue(ops, d["x"], d["gy"], kw, "prelu", 0.2, 9, vec=True))
    layer_norm_against_the_mirror(mirror, d, kw, flags, 0.2, 9, *device_layer_norm(ops, off, d["gy"], kw, "prelu", 0.2, 9, False, INSTANCE[f]))
    layer_norm_against_the_mirror(mirror, d, kw, flags, 0.2, 9, *device_layer_norm(ops, d["x"], d["gy"], kw, "prelu", 0.2, 9, True, INSTANCE[f]))


def test_every_strided_launch_takes_a_second_round(mirror, ops):
    c = rm.constants(mirror)
    L, n, f = c["max_grid"] * c["group_waves"] + 1, 2, 4
    assert L == 8193
    d = rm.inputs(L, n, f, 11)
    kw, flags = arguments(d, f, "prelu", False, True)
    epilogue_against_the_mirror(mirror, d, kw, flags, 0.2, 3, *device_epilogue(ops, d["x"], d["gy"], kw, "prelu", 0.2, 3, vec=True))
    # the layer norm's column sums and finishing kernel stride as the epilogue's do; its row kernel takes 64 rows a wave at F = 4 ...
    layer_norm_against_the_mirror(mirror, d, kw, flags, 0.2, 3, *device_layer_norm(ops, d["x"], d["gy"], kw, "prelu", 0.2, 3, True, 1))
    # ... and one row a wave at F = 260, where 8,193 rows are a second round
    wide = rm.inputs(1, 8193, 260, 12)
    kw, flags = arguments(wide, 260, "relu", False, False)
    layer_norm_against_the_mirror(mirror, wide, kw, flags, 0.0, 0, *device_layer_norm(ops, wide["x"], wide["gy"], kw, "relu", 0.0, 0, True, 2))


def test_a_nan_stays_in_its_place(mirror, ops):
    """Without activations, so that the NaN is not compared away (v > 0 is false for it)."""
    L, n, f = 1, 257, 8
    d = rm.inputs(L, n, f, 13)
    kw, flags = arguments(d, f, "none", False, True)
    clean_e = device_epilogue(ops, d["x"], d["gy"], kw, "none", 0.0, 0, True)
    clean_l = device_layer_norm(ops, d["x"], d["gy"], kw, "none", 0.0, 0, True, 1)
    d["x"][0, 100, 5] = np.nan
    y, grads = device_epilogue(ops, d["x"], d["gy"], kw, "none", 0.0, 0, True)
    got, ref = y.detach().cpu().numpy(), clean_e[0].detach().cpu().numpy()
    assert np.isnan(got[0, 100, 5]) and np.isnan(got).sum() == 1
    got[0, 100, 5] = ref[0, 100, 5]
    assert same_bits(got, ref) and same_bits(grads["gx"], clean_e[1]["gx"]) and same_bits(grads["gbias"], clean_e[1]["gbias"])
    y, grads = device_layer_norm(ops, d["x"], d["gy"], kw, "none", 0.0, 0, True, 1)
    m = rm.ln_forward(mirror, d["x"], kw["weight"], kw["bias"], None, 1e-5, 0.0, 0, flags)[0]
    rows = [i for i in range(n) if i != 100]
    for got, ref in ((y, clean_l[0]), (grads["gx"], clean_l[1]["gx"])):
        got = got.detach().cpu().numpy()
        assert np.isnan(got[0, 100]).all() and same_bits(got[:, rows], ref.detach().cpu().numpy()[:, rows])
    assert np.array_equal(y.detach().cpu().numpy(), m, equal_nan=True)


def test_layers_repeat_and_the_backward_pass_draws_the_mask_again(ops):
    L, n, f = 3, 513, 33
    d = rm.inputs(L, n, f, 17)
    kw, _ = arguments(d, f, "prelu", True, True)
    d["x"][d["x"] == 0] = 0.5           # (so that y == 0 marks a dropped element)
    d["gy"][d["gy"] == 0] = 0.5

    def run(x, gy, seed, call):
        tx = cuda(x, True)
        w, b, s = (cuda(kw[k], True) for k in ("weight", "bias", "slope"))
        if call == "epilogue":
            y = ops.bias_act_dropout(tx, b, act="prelu", slope=s, p=0.3, seed=seed)
        else:
            y = ops.layer_norm(tx, w, b, post="prelu", slope=s, p=0.3, seed=seed)
        y.backward(cuda(gy))
        return y, tx.grad, b.grad, s.grad

    for call in ("epilogue", "layer_norm"):
        one, two = run(d["x"], d["gy"], 50, call), run(d["x"], d["gy"], 50, call)
        assert all(same_bits(a, b) for a, b in zip(one, two))
        assert not same_bits(one[0], run(d["x"], d["gy"], 51, call)[0])
        dropped = one[0].detach() == 0
        assert 0.25 < float(dropped.float().mean()) < 0.35
        if call == "epilogue":   # (a layer norm's gx mixes the row: only the epilogue's is zero where y was dropped)
            assert bool((one[1][dropped] == 0).all()) and bool((one[1][~dropped] != 0).all())
        for l in range(L):
            y, gx = run(d["x"][l], d["gy"][l], 50 + l, call)[:2]
            assert y.shape == (n, f) and same_bits(y, one[0][l]) and same_bits(gx, one[1][l])


def test_no_dropout_gives_the_bits_of_the_call_without_it(ops):
    d = rm.inputs(2, 100, 32, 19)
    x, b, s = cuda(d["x"]), cuda(d["bias"]), cuda(d["slope"])
    base = ops.bias_act_dropout(x, b, act="prelu", slope=s)
    assert same_bits(base, ops.bias_act_dropout(x, b, act="prelu", slope=s, p=0.4, training=False, seed=3))
    ln = ops.layer_norm(x, post="relu")
    assert same_bits(ln, ops.layer_norm(x, post="relu", p=0.4, training=False, seed=None))
    assert not same_bits(ln, ops.layer_norm(x, post="relu", p=0.4, seed=3))


# ------------------------------------------------------------------------------------------------ end to end
GRAPH_NODES, IN, HID, LAYERS = [40, 40, 40], 5, 8, 2


def snapshots():
    from rlap_amd import adapters, graphs
    node_ptr = [0] + list(np.cumsum(GRAPH_NODES))
    eis = [graphs.barabasi_albert(ng, 2, 30 + g) + node_ptr[g] for g, ng in enumerate(GRAPH_NODES)]
    n = node_ptr[-1]
    x = torch.from_numpy(np.random.RandomState(3).uniform(-1, 1, size=(n, IN))).float().cuda()
    aug = adapters.rLapViews(fracs=(0.2, 0.4), o_v="random", o_n="asc", keep_weights=False, seed=5)
    return x, aug.snapshots((x, torch.cat(eis, dim=1).cuda(), None), node_ptr=node_ptr), n


def f64(t):
    return t.detach().cpu().double()


@pytest.mark.parametrize("norm", ["batch", "layer"])
def test_g2l_encoder_end_to_end(ops, norm):
    from rlap_amd import adapters
    x, holder, n = snapshots()
    planned = holder.plan()
    torch.manual_seed(6)
    enc = adapters.SnapshotG2LEncoder(IN, HID, LAYERS, dropout=0.2, encoder_norm=norm, projector_norm=norm, seed=77).cuda()
    up = lambda t: torch.linspace(-1, 1, t.numel(), device=t.device).reshape(t.shape)

    def step():
        for p in enc.parameters():
            p.grad = None
        for m in enc.modules():
            if isinstance(m, adapters.SnapshotBatchNorm):
                m.reset_parameters()
        z, proj = enc(x, planned)
        ((z * up(z)).sum() + (proj * up(proj)).sum()).backward()
        return [z.detach(), proj.detach()] + [p.grad.clone() for p in enc.parameters()]

    one, two = step(), step()
    assert one[0].shape == one[1].shape == (2, n, HID)
    assert all(same_bits(a, b) for a, b in zip(one, two))                                   # equal bits twice under a fixed seed
    assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in enc.parameters())   # every parameter reached
    assert float((one[1] == 0).float().mean()) > 0.1                                        # the head's dropout is on
    free = adapters.SnapshotG2LEncoder(IN, HID, LAYERS, dropout=0.2, encoder_norm=norm, projector_norm=norm).cuda()
    with torch.no_grad():
        a, b = free(x, planned)[1], free(x, planned)[1]
    assert not same_bits(a == 0, b == 0)                                                    # seed=None: different masks on consecutive calls

    # eval(): no dropout, and the output within the float32 format bound of a float64 torch restatement, layer by layer on what
    # each module was given (hooks), so that each bound is one module's
    enc.eval()
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, args, out, key=key: seen.__setitem__(key, (args[0].detach(), out.detach())))
             for key, m in (("norm", enc.batch_norm), ("head", enc.head_norm))]
    with torch.no_grad():
        z, proj = enc(x, planned)
        again = enc(x, planned)
    for h in hooks:
        h.remove()
    assert same_bits(z, again[0]) and same_bits(proj, again[1]) and same_bits(z, seen["norm"][1])
    for key, mod in (("norm", enc.batch_norm), ("head", enc.head_norm)):
        zin, zout = f64(seen[key][0]), f64(seen[key][1])
        if norm == "layer":
            v = torch.nn.functional.layer_norm(zin, (HID,), f64(mod.weight), f64(mod.bias), mod.eps)
            xh = torch.nn.functional.layer_norm(zin, (HID,), None, None, mod.eps)
        else:
            rstd = 1.0 / torch.sqrt(f64(mod.running_var) + mod.eps)
            xh = (zin - f64(mod.running_mean)) * rstd
            v = xh * f64(mod.weight) + f64(mod.bias)
        want = torch.where(v > 0, v, f64(mod.slope) * v) if key == "head" else v
        size = xh.abs() * f64(mod.weight).abs() + f64(mod.bias).abs()
        assert bool(((zout - want).abs() <= 2.0 ** -24 * want.abs() + 1e-13 * size).all()), key


def test_gcn_conv_with_an_epilogue(mirror, ops):
    from rlap_amd import adapters
    x, holder, n = snapshots()
    torch.manual_seed(8)
    plain = adapters.SnapshotGCNConv(IN, HID).cuda()
    fused = adapters.SnapshotGCNConv(IN, HID, epilogue=adapters.SnapshotActDropout("prelu", 0.2, seed=21)).cuda()
    fused.load_state_dict(plain.state_dict(), strict=False)
    with torch.no_grad():
        plain.bias.copy_(torch.linspace(-0.5, 0.5, HID))
        fused.bias.copy_(plain.bias)
    with torch.no_grad():
        prop = holder.propagate(x @ plain.weight)
        assert same_bits(plain(x, holder), prop + plain.bias)                               # without the epilogue: what it was
    y = fused(x, holder)
    flags = rm.flags_of("prelu", False, True)
    want = rm.forward(mirror, prop.cpu().numpy(), plain.bias.detach().cpu().numpy(), np.array([0.25], dtype=np.float32), 0.2, 21, flags)
    assert same_bits(y, want) and same_bits(y, fused(x, holder))
    y.sum().backward()
    assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in fused.parameters())
    fused.eval()
    with torch.no_grad():
        ev = fused(x, holder)
    v = f64(prop) + f64(plain.bias)
    want = torch.where(v > 0, v, 0.25 * v)
    assert bool(((f64(ev) - want).abs() <= 2.0 ** -24 * want.abs()).all())
