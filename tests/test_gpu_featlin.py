"""The sparse first layer on the device (ops.feature_plan / FeaturePlan.linear) against its two yardsticks: the host
mirror (tests/csrc/featlin_mirror.cc, bit for bit) and the dense float64 products (within the bound of tests/test_featlin_cpu.py:
bound_factor(T, True) * A with T the terms of the longest sum, plus 2^-24 (|ref| + bound) for a float32 result).

Paths.  The crafted 520 x 520 matrix has rows and columns of 0, 1, 255, 256, 257 and 513 entries: the one-chunk and the chunked
walks of the forward kernel, the chunk kernel and both branches of the transposed row kernel (scratch_entries 0, 1, default).  Fout
1 and 3 take the scalar path with one and four lanes, 4, 64, 68 and 256 the vector path (1, 16, 17 and 64 lanes), 260 (65 vector
lanes) two feature tiles; a weight shifted by one element the alignment fallback.  K 1, 2 run the 1- and 2-view kernels, 8 the
8-view one, 9 and 32 two and four groups of 8 (K 3 and 4 in the small shapes the 4-view one).
"""
import numpy as np
import pytest
import torch

import featlin_mirror as fm
from test_gpu_propagate import bound_factor

pytestmark = pytest.mark.gpu

NP = {torch.float32: np.float32, torch.float64: np.float64}


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops
    mirror = fm.build(tmp_path_factory.mktemp("featlin"))
    out = {"mirror": mirror, "ops": ops}
    for dt in (torch.float32, torch.float64):
        x = fm.crafted(NP[dt])
        out[dt] = {"x": x, "fp": ops.feature_plan(torch.from_numpy(x).cuda()), "plan": fm.plan(mirror, x)}
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check_plan(env, fp, x, directions="both"):
    """The device plan equals the mirror's part by part, and reports the mirror's counts."""
    p = fm.plan(env["mirror"], x, directions)
    assert fp.nnz == p["desc"]["nnz"] and fp.nbytes == p["desc"]["plan_bytes"] and (fp.num_nodes, fp.in_features) == x.shape
    for k in fm.DESC:
        assert getattr(fp.desc, k) == p["desc"][k], k
    assert fm.same_parts(fm.decode(host(fp.buffer), fp.desc), fm.decode(p["buffer"], p["desc"]))
    f, t = fm.DIRS[directions]
    kept = (x.astype(np.float64) != 0.0)
    lens = {"forward": kept.sum(1), "transposed": kept.sum(0)}
    for name, has in (("forward", f), ("transposed", t)):
        if not has:
            assert fp.info["longest_" + name] == fp.info["long_lists_" + name] == fp.info["chunks_" + name] == -1
            continue
        n = lens[name]
        assert fp.info["longest_" + name] == p["info"]["longest_" + name] == int(n.max())
        assert fp.info["long_lists_" + name] == p["info"]["long_lists_" + name] == int((n > fm.CHUNK).sum())
        assert fp.info["chunks_" + name] == p["desc"]["chunks_" + name] == int(((n[n > fm.CHUNK] + fm.CHUNK - 1) // fm.CHUNK).sum())
    assert fp.info["nnz"] == fp.nnz and fp.info["host_syncs"] == 1
    return p


def check_products(env, fp, p, x, K, wdt, kind, Fout, shifted=False, seed=0):
    """Both products of one case against the mirror (bits) and the dense float64 reference (bound); what the issue lists."""
    ops = env["ops"]
    rng = np.random.default_rng(seed + 1000 * K + Fout)
    N, Fin = x.shape
    keep = None if kind is None else fm.masks(kind, K, x, seed=seed + K)
    w = rng.uniform(-1, 1, size=(Fin, Fout)).astype(NP[wdt])
    g = rng.uniform(-1, 1, size=(K, N, Fout)).astype(NP[wdt])
    if shifted:   # a view one element into a larger allocation: contiguous, not 16-byte aligned
        d_w = torch.empty(Fin * Fout + 1, dtype=wdt, device="cuda")[1:].view(Fin, Fout).copy_(dev(w))
        d_g = torch.empty(K * N * Fout + 1, dtype=wdt, device="cuda")[1:].view(K, N, Fout).copy_(dev(g))
        assert d_w.data_ptr() % 16 != 0 and d_g.data_ptr() % 16 != 0
    else:
        d_w, d_g = dev(w), dev(g)
    d_keep = None if keep is None else dev(keep)
    lf, lt = max(int(fp.info["longest_forward"]), 1), max(int(fp.info["longest_transposed"]), 1)
    # forward
    y = fp.linear(d_w, d_keep)
    assert ops.last_stats["host_syncs"] == 0
    y3 = host(y) if keep is not None else host(y)[None]
    assert fm.same_bits(y3, fm.apply(env["mirror"], p, w, keep)), "y differs from the mirror"
    ref, A = fm.reference(x, w, keep, False)
    ok, worst = fm.within_bound(y3, ref, A, bound_factor(lf, True))
    print(f"forward K={K} {wdt} {kind} Fout={Fout}: worst |y - ref| / bound = {worst:.3e}")
    assert ok, worst
    assert not y3[A == 0].any() and not np.signbit(y3[A == 0]).any()                          # nothing kept: exactly +0.0
    assert fm.same_bits(host(fp.linear(d_w, d_keep)), host(y))                                 # the same bits on every run
    if keep is not None:
        for k in sorted({0, K // 2, K - 1}):                                                  # view k alone, with mask k
            assert fm.same_bits(host(fp.linear(d_w, d_keep[k:k + 1]))[0], y3[k]), f"view {k}"
    # transposed: G -> dW through the autograd function's call
    dws = []
    for limit in (0, 1, -1):
        ops.debug_set_limits(scratch_entries=limit)
        try:
            dws.append(host(ops._feature_apply(fp, d_g, d_keep, K, True)))
        finally:
            ops.debug_set_limits(scratch_entries=-1)
    assert fm.same_bits(dws[0], dws[2]) and fm.same_bits(dws[1], dws[2]), "dW depends on the chunk-sum budget"
    assert fm.same_bits(dws[2], fm.apply(env["mirror"], p, g, keep, transpose=True)), "dW differs from the mirror"
    ref, A = fm.reference(x, g, keep, True)
    ok, worst = fm.within_bound(dws[2], ref, A, bound_factor(lt * K, True))
    print(f"transposed K={K} {wdt} {kind} Fout={Fout}: worst |dW - ref| / bound = {worst:.3e}")
    assert ok, worst
    assert not dws[2][A == 0].any() and not np.signbit(dws[2][A == 0]).any()
    assert fm.same_bits(host(ops._feature_apply(fp, d_g, d_keep, K, True)), dws[2])


@pytest.mark.parametrize("xdt", [torch.float32, torch.float64])
def test_crafted_plan_equals_the_mirror(env, xdt):
    c = env[xdt]
    check_plan(env, c["fp"], c["x"])
    assert c["fp"].info["longest_forward"] == c["fp"].info["longest_transposed"] == 513
    assert c["fp"].info["chunks_forward"] == c["fp"].info["chunks_transposed"] == 5           # the chunk paths run below
    for d in ("forward", "transposed"):
        check_plan(env, env["ops"].feature_plan(dev(c["x"]), d), c["x"], d)


def test_special_values_are_entries_as_the_rule_says(env):
    x = fm.crafted_with_nan(np.float32)
    fp = env["ops"].feature_plan(dev(x))
    p = check_plan(env, fp, x)                                                                 # -0.0 dropped; the denormal and the NaN kept
    w = np.random.default_rng(2).uniform(-1, 1, size=(520, 4)).astype(np.float32)
    keep = fm.masks("random", 2, x)
    assert fm.same_bits(host(fp.linear(dev(w), dev(keep))), fm.apply(env["mirror"], p, w, keep))
    assert np.isnan(host(fp.linear(dev(w)))[4]).all()


# K, x type, weight type, masks, Fout, shifted weight: every K, Fout, mask kind and type pair at least once
CASES = [
    (1, torch.float32, torch.float32, None, 1, False), (1, torch.float32, torch.float32, "all", 260, False),
    (2, torch.float32, torch.float32, "random", 256, False), (2, torch.float32, torch.float64, "chunk", 3, False),
    (2, torch.float64, torch.float32, "none", 4, False), (8, torch.float32, torch.float32, "chunk", 64, False),
    (8, torch.float64, torch.float64, "random", 68, False), (9, torch.float32, torch.float32, "random", 68, True),
    (9, torch.float64, torch.float64, "chunk", 4, True), (32, torch.float32, torch.float32, "random", 4, False),
    (32, torch.float32, torch.float64, "all", 3, False), (2, torch.float32, torch.float64, "random", 260, False),
    (1, torch.float64, torch.float32, "random", 64, True), (8, torch.float32, torch.float32, "none", 1, False),
]


@pytest.mark.parametrize("K,xdt,wdt,kind,Fout,shifted", CASES)
def test_crafted_products(env, K, xdt, wdt, kind, Fout, shifted):
    c = env[xdt]
    check_products(env, c["fp"], c["plan"], c["x"], K, wdt, kind, Fout, shifted)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("Fin", [1, 7, 257])
def test_small_shapes(env, N, Fin):
    xdt = torch.float32 if (N + Fin) % 2 else torch.float64
    x = fm.random_sparse(N, Fin, min(Fin, 260), NP[xdt], seed=N + Fin)
    fp = env["ops"].feature_plan(dev(x))
    p = check_plan(env, fp, x)
    K, Fout = (3, 3) if N % 2 else (4, 4)
    check_products(env, fp, p, x, K, torch.float32 if Fin != 7 else torch.float64, "random", Fout, seed=N)


def test_autograd_is_the_transposed_call(env):
    ops, c = env["ops"], env[torch.float32]
    x, fp = c["x"], c["fp"]
    rng = np.random.default_rng(8)
    keep = dev(fm.masks("random", 2, x))
    for d_keep, K in ((keep, 2), (None, 1)):
        w = dev(rng.uniform(-1, 1, size=(520, 12)).astype(np.float32)).requires_grad_()
        r = dev(rng.uniform(-1, 1, size=(K, 520, 12)).astype(np.float32))
        y = fp.linear(w, d_keep)
        ((y if d_keep is not None else y[None]) * r).sum().backward()
        assert fm.same_bits(host(w.grad), host(ops._feature_apply(fp, r, d_keep, K, True)))
    fwd = ops.feature_plan(dev(x), "forward")
    w = dev(rng.uniform(-1, 1, size=(520, 4)).astype(np.float32)).requires_grad_()
    y = fwd.linear(w)
    with pytest.raises(RuntimeError, match="transposed"):
        y.sum().backward()
    assert not fwd.linear(w.detach()).requires_grad


def test_gradcheck_float64(env):
    x = fm.random_sparse(5, 7, 4, np.float64, seed=4)
    fp = env["ops"].feature_plan(dev(x))
    keep = dev(fm.masks("random", 2, x))
    w = torch.randn(7, 3, dtype=torch.float64, device="cuda", requires_grad=True)
    assert torch.autograd.gradcheck(lambda w_: fp.linear(w_, keep), (w,), eps=1e-6, atol=1e-8, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda w_: fp.linear(w_), (w,), eps=1e-6, atol=1e-8, nondet_tol=0.0)


def test_gcn_conv_over_a_feature_plan(env):
    """conv(fp, snaps, keep) is snaps.propagate(fp.linear(W, keep)) + b.  The float64 restatement of the whole layer is
    A_l ((x * keep[l]) W) + b with A_l[j][i] the summed weights of layer l's rows i -> j; the bound is the first product's, carried
    through |A_l|, plus the second product's over |A_l| (|z| + bound1), each with its float32 rounding, plus the bias add's."""
    from rlap_amd import adapters
    ops = env["ops"]
    c = env[torch.float32]
    x, fp = c["x"], c["fp"]
    rng = np.random.default_rng(21)
    N, L, m = 520, 2, 3000
    rows = np.stack([rng.integers(0, N, size=m), rng.integers(0, N, size=m), rng.uniform(0.5, 1.5, size=m)], 1).astype(np.float64)
    snaps = ops.edge_list_plan(dev(rows), [0, 1400, m], N, weighted=True, add_self_loops=False, normalize=False)
    keep = fm.masks("random", L, x)
    torch.manual_seed(3)
    conv = adapters.SnapshotGCNConv(520, 20).cuda()
    with torch.no_grad():
        conv.bias.uniform_(-1, 1)
    out = conv(fp, snaps, keep=dev(keep))
    assert out.shape == (L, N, 20)
    with torch.no_grad():
        assert torch.equal(out, snaps.propagate(fp.linear(conv.weight, dev(keep))) + conv.bias)
    out.sum().backward()
    assert conv.weight.grad is not None and conv.bias.grad is not None and bool(conv.weight.grad.abs().sum() > 0)
    assert torch.equal(conv.bias.grad, torch.full((20,), float(L * N), device="cuda"))
    w, b = host(conv.weight).astype(np.float64), host(conv.bias).astype(np.float64)
    z, A1 = fm.reference(x, w, keep, False)
    b1 = bound_factor(513, True) * A1
    b1 = b1 + 2.0 ** -24 * (np.abs(z) + b1)
    for l, (lo, hi) in enumerate(((0, 1400), (1400, m))):
        A = np.zeros((N, N))
        np.add.at(A, (rows[lo:hi, 1].astype(int), rows[lo:hi, 0].astype(int)), rows[lo:hi, 2])
        longest = int(np.bincount(rows[lo:hi, 1].astype(int), minlength=N).max())
        ref = A @ z[l] + b
        mag = np.abs(A) @ (np.abs(z[l]) + b1[l])
        b2 = bound_factor(longest, True) * mag
        b2 = b2 + 2.0 ** -24 * (mag + b2)
        bound = np.abs(A) @ b1[l] + b2 + 2.0 ** -24 * (np.abs(ref) + np.abs(A) @ b1[l] + b2)
        err = np.abs(host(out)[l].astype(np.float64) - ref)
        print(f"layer {l}: worst error / bound = {float((err / bound).max()):.3e}")
        assert (err <= bound).all()
    with pytest.raises(ValueError, match="keep goes with"):
        conv(dev(x), snaps, keep=dev(keep))
