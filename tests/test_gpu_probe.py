"""The linear-probe evaluator on the device (ops.linear_probe / ops.probe_scores, rlap_linear_probe / rlap_probe_scores)
against its host mirror (tests/csrc/probe_mirror.cc around rlap_amd/csrc/rlap_probe.h, the header the kernels include).

Shapes: F at the edges of the 256 columns a thread pass covers and of odd / even row strides (1, 3, 31, 32, 33, 64, 300, 512), C
at the edges of every class padding (2, 3, 7 -> 8; 16; 32; 33, 64 -> 64), n_train at the edges of the 32-row tile (1, 31, 32, 33,
45), of the 256-row chunk and of the part split (257: two parts, 600: three), in a sparse cross product; epochs <= 60,
test_interval in {1, 5, 20}, both selection rules, weight_decay in {0, 1e-4}.  The mirror runs once per case (a module-wide cache).

  bit for bit   weight, bias, confusion, every score, best_epoch and best_val_correct equal the mirror's bits: the parameter
                trajectory holds IEEE operations only (a float32 quotient and root are formed in float64 and rounded once).
  loss          the device's float64 log is not the host's, so the loss is compared element by element within LOSS_LOG_BOUND
                relative: four times the largest difference measured over these cases on an MI355X against the mirror.  That
                difference is 0 -- on these inputs the two logarithms agree in every bit -- so the bound is equality.
"""
import numpy as np
import pytest
import torch

import probe_mirror as pm

pytestmark = pytest.mark.gpu

LOSS_LOG_BOUND = 4 * 0.0

# (n_train, F, C, R, epochs, test_interval, select, weight_decay, overlap)
CASES = [
    (1, 1, 2, 1, 20, 1, "scripts", 0.0, False),
    (31, 3, 3, 1, 40, 5, "cca", 1e-4, False),
    (32, 31, 7, 3, 40, 20, "scripts", 1e-4, False),
    (33, 32, 32, 1, 20, 5, "scripts", 0.0, True),
    (300, 33, 33, 1, 20, 20, "cca", 0.0, False),
    (257, 64, 64, 3, 20, 5, "scripts", 1e-4, True),
    (45, 512, 64, 1, 20, 20, "scripts", 0.0, False),
    (600, 300, 7, 1, 20, 5, "cca", 1e-4, False),
    (33, 512, 2, 3, 60, 20, "scripts", 0.0, False),
    (300, 64, 16, 1, 20, 1, "scripts", 0.0, False),
]
IDS = [f"n{c[0]}-F{c[1]}-C{c[2]}-R{c[3]}-{c[6]}" for c in CASES]
KEYS_BITS = ("weight", "bias", "confusion", "micro_f1", "macro_f1", "accuracy", "best_epoch", "best_val_correct")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import ops as o
    return o


def problem(nt, f, c, r, overlap, seed=None):
    """x, y, the runs' ragged lists (run k trains on nt + 3 k rows, in a shuffled order) and the initial parameters."""
    seed = 7000 + 13 * nt + f + c if seed is None else seed
    extra = max(48, 3 * c)
    n = nt + 3 * r + 2 * extra + 5
    x, y = pm.blobs(n, f, c, seed)
    rng = np.random.RandomState(seed + 1)
    train, valid, test = [], [], []
    for k in range(r):
        perm = rng.permutation(n)
        ntk = nt + 3 * k
        train.append(perm[:ntk])
        rest = perm[:] if overlap else perm[ntk:]
        valid.append(rest[:extra - 7 * k])
        test.append(rest[extra - 7 * k:2 * extra + k])
    w0, b0 = pm.init(r, c, f, seed + 2)
    return x, y, train, valid, test, w0, b0


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    lib = pm.build(tmp_path_factory.mktemp("probe"))
    cache = {}

    def get(case):
        if case not in cache:
            nt, f, c, r, epochs, interval, select, wd, overlap = case
            x, y, tr, va, te, w0, b0 = problem(nt, f, c, r, overlap)
            cache[case] = pm.run(lib, x, y, tr, va, te, w0, b0, epochs, weight_decay=wd, test_interval=interval, select=select)
        return cache[case]
    get.lib = lib
    return get


def bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x).tobytes()


def same(name, got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    if bits(got) != bits(want):
        bad = np.argwhere(got != want)
        first = tuple(bad[0]) if bad.size else None
        raise AssertionError(f"{name}: {len(bad)} elements differ" + (f", first at {first}: {got[first]!r} != {want[first]!r}" if bad.size else " (sign of zero / NaN)"))


def device_call(ops, case, x=None, **kw):
    nt, f, c, r, epochs, interval, select, wd, overlap = case
    x0, y, tr, va, te, w0, b0 = problem(nt, f, c, r, overlap)
    xd = torch.from_numpy(x0).cuda() if x is None else x
    t = lambda lists: [torch.from_numpy(a).cuda() for a in lists]
    return ops.linear_probe(xd, torch.from_numpy(y).cuda(), t(tr), t(va), t(te), num_classes=c, epochs=epochs, weight_decay=wd,
                            test_interval=interval, select=select, weight=torch.from_numpy(w0), bias=torch.from_numpy(b0), **kw)


def check(res, m, what=""):
    assert int(res["status"]) == 0 and m["status"] == 0
    for key in KEYS_BITS:
        same(what + key, res[key], m[key])
    loss = res["loss"].cpu().numpy()
    rel = np.abs(loss - m["loss"]) / np.abs(m["loss"])
    print(f"{what}loss relative difference to the mirror: {rel.max():.3g}")
    assert (rel <= LOSS_LOG_BOUND).all(), (loss, m["loss"])


def test_the_cases_cover_the_paddings_the_tiles_and_the_part_split(mirror):
    lib = mirror.lib
    assert sorted({lib.probe_class_pad(c[2]) for c in CASES}) == [8, 16, 32, 64]
    assert {f for _, f, *_ in CASES} >= {1, 3, 31, 32, 33, 64, 512} and {c[2] for c in CASES} >= {2, 3, 7, 32, 33, 64}
    assert {c[0] for c in CASES} >= {1, 31, 32, 33, 300}
    assert lib.probe_parts(257, 64, 64) == 2 and lib.probe_parts(600, 300, 7) == 3 and lib.probe_parts(300, 33, 33) == 2
    assert {c[5] for c in CASES} == {1, 5, 20} and all(c[4] <= 60 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_equals_the_mirror_bit_for_bit(ops, mirror, case):
    res = device_call(ops, case)
    st = dict(ops.last_stats)
    assert st["host_syncs"] == 0 and st["runs"] == case[3] and st["detail"] == 0
    check(res, mirror(case))
    assert int(res["best_val_correct"].max()) > 0          # (something was recorded: the comparison above is not one of zeros)


def test_poisoned_arena_and_padding_rows_change_no_bit(ops, mirror):
    """n_train = 45 and 257 + 3 k are no multiples of 32: the rows that fill the last tile, the arena and the result buffers hold
    0xFF bytes (NaNs) before the call."""
    ops.debug_set_poison(0xFF)
    try:
        for case in (CASES[6], CASES[5]):
            check(device_call(ops, case), mirror(case), "poisoned ")
    finally:
        ops.debug_set_poison(-1)


def test_two_calls_and_a_call_after_unrelated_calls_return_equal_bits(ops, mirror):
    case = CASES[5]
    first = device_call(ops, case)
    second = device_call(ops, case)
    a = torch.randn(300, 64, device="cuda")
    ops.cca_loss(a, a * 0.5 + torch.randn_like(a), 1e-3)  # (leaves other data in the workspace)
    ops.info_nce(a, torch.randn_like(a), 0.4)
    third = device_call(ops, case)
    for key in KEYS_BITS + ("loss",):
        same("second " + key, second[key], first[key].cpu().numpy())
        same("third " + key, third[key], first[key].cpu().numpy())


def test_a_strided_view_of_x_is_read_in_place_or_copied_never_wrongly(ops, mirror):
    for case in (CASES[2], CASES[4]):
        nt, f, c, r, *_ , overlap = case
        x0 = problem(nt, f, c, r, overlap)[0]
        wide = torch.full((x0.shape[0] + 2, f + 5), float("nan"), device="cuda")
        wide[1:-1, 3:3 + f] = torch.from_numpy(x0).cuda()
        check(device_call(ops, case, x=wide[1:-1, 3:3 + f]), mirror(case), "offset view ")               # rows f + 5 floats apart
        tall = torch.from_numpy(np.ascontiguousarray(x0.T)).cuda().t()                                     # column-major
        assert tall.stride(1) != 1 or f == 1
        check(device_call(ops, case, x=tall), mirror(case), "transposed view ")


def test_runs_in_one_call_equal_single_calls(ops, mirror):
    case = CASES[5]
    nt, f, c, r, epochs, interval, select, wd, overlap = case
    x, y, tr, va, te, w0, b0 = problem(nt, f, c, r, overlap)
    m = mirror(case)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for k in range(r):
        one = ops.linear_probe(xd, yd, torch.from_numpy(tr[k]).cuda(), torch.from_numpy(va[k]).cuda(), torch.from_numpy(te[k]).cuda(),
                               num_classes=c, epochs=epochs, weight_decay=wd, test_interval=interval, select=select,
                               weight=torch.from_numpy(w0[k:k + 1]), bias=torch.from_numpy(b0[k:k + 1]))
        for key in KEYS_BITS:
            same(f"run {k} {key}", one[key], m[key][k:k + 1])


def test_probe_scores_against_the_mirror_ties_included(ops, mirror):
    """Equal rows of W give equal logits: the prediction is the lowest index among them."""
    n, f, c = 150, 33, 7
    x, y = pm.blobs(n, f, c, 31)
    w, b = pm.init(3, c, f, 32)
    w[0, 5] = w[0, 2]; b[0, 5] = b[0, 2]
    w[1, :] = w[1, 0]; b[1, :] = b[1, 0]                       # every logit equal: class 0 everywhere
    rng = np.random.RandomState(33)
    index = [rng.permutation(n)[:k] for k in (150, 33, 1)]
    m = pm.scores(mirror.lib, x, y, index, w, b)
    res = ops.probe_scores(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), [torch.from_numpy(a).cuda() for a in index],
                           torch.from_numpy(w), torch.from_numpy(b))
    assert int(res["status"]) == 0
    for key in ("pred", "confusion", "micro_f1", "macro_f1", "accuracy"):
        same(key, res[key], m[key])
    pred = res["pred"].cpu().numpy()
    assert not (pred[:150] == 5).any() and (pred[150:183] == 0).all()
    acc, micro, macro, conf = pm.numpy_scores(y[index[0]], pred[:150], c)
    assert np.array_equal(conf, m["confusion"][0]) and macro == pytest.approx(float(res["macro_f1"][0]), abs=1e-15)


def test_evaluate_runs_equals_the_per_run_calls(ops):
    from rlap_amd import adapters
    n, f, c = 200, 16, 4
    x, y = pm.blobs(n, f, c, 41)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    splits = adapters.get_split(n, runs=3, generator=torch.Generator().manual_seed(5))
    ev = lambda: adapters.LREvaluator(num_epochs=40, test_interval=5, generator=torch.Generator().manual_seed(6))
    together = ev().evaluate_runs(xd, yd, splits)
    single = ev()
    alone = [single.evaluate(xd, yd, s) for s in splits]      # (one generator: the same draws in the same order)
    assert together == alone and all(set(d) == {"micro_f1", "macro_f1", "accuracy"} for d in together)
    assert all(isinstance(v, float) for d in together for v in d.values()) and together[0]["accuracy"] > 0.5


def test_bad_indices_and_labels_are_reported_and_never_dereferenced(ops):
    n, f, c = 64, 8, 3
    x, y = pm.blobs(n, f, c, 51)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    idx = torch.arange(n, device="cuda")
    bad = idx.clone(); bad[5] = n + 10 ** 9
    res = ops.linear_probe(xd, yd, bad, idx, idx, num_classes=c, epochs=2, test_interval=1, generator=torch.Generator().manual_seed(1))
    assert int(res["status"]) == 2
    res = ops.linear_probe(xd, yd, idx, idx, idx, num_classes=2, epochs=2, test_interval=1, generator=torch.Generator().manual_seed(1))
    assert int(res["status"]) == 3                            # labels reach 2 with two classes
