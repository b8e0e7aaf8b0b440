"""The linear-probe evaluator (ops.linear_probe / ops.probe_scores, rlap_linear_probe / rlap_probe_scores) without a GPU:

  * the rule -- the host mirror (tests/csrc/probe_mirror.cc, every value from rlap_amd/csrc/rlap_probe.h, contraction off) against a
    float64 torch restatement of LREvaluator's loop (scripts/node_shared.py:163-230) and of CCA-SSG/main.py:152-194's, with
    torch.optim.Adam in float64 from the same initial parameters: parameters, loss and predictions after 1, 20 and 200 epochs;
  * the scores against numpy and, where it imports, sklearn; the order's invariances;
  * the index arithmetic of the header in a stand-alone program under -fsanitize=address,undefined, exhaustively for n_train <= 600;
  * the Python -> C mapping of both exports on a stub library, the layout of rlap_probe_info, adapters.LREvaluator and get_split,
    the argument errors.

The bounds of the first group are four times the largest differences measured with these inputs (DESIGN 4.18 has the figures).
Measured here: parameters 1.03e-3 of the largest parameter (n_train = 129, F = 512, C = 64, weight_decay = 1e-4, after ONE epoch: Adam's
first step is lr * g / (|g| + eps), the size of lr whatever the size of g, so a gradient entry of the size of eps = 1e-8 -- two rows a
class and 32,768 entries have some -- turns a float32 gradient's last bits into a good part of lr; every shape with fewer classes
measures at most 1.44e-6); loss 1.32e-5 relative (the same shape after 200 epochs, a loss of 9e-7; at most 2.26e-6 with fewer classes);
logits at the last epoch 2.87e-4 absolute (the same shape; 4.7e-6 at most with fewer classes).  A prediction is left out of the
comparison only where the restatement's gap between its two largest logits is below four times the logit difference measured for its
case, at most 1 % of a set's rows (the sets hold 200 rows or more); with these inputs no prediction that is compared differs.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import probe_mirror as pm
from rlap_amd import _lib, adapters, ops
from test_cabi_symbols import test_layout_matches_the_header as layout_matches_the_header
from util import StubLib, i64_at, stub_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAM_BOUND = 4 * 1.03e-3    # relative to the largest parameter
LOSS_BOUND = 4 * 1.32e-5     # relative to the loss
LOGIT_BOUND = 4 * 2.87e-4    # absolute, at the last epoch


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    return pm.build(tmp_path_factory.mktemp("probe"))


# ------------------------------------------------------------------------------------------------ the rule
SHAPES = [(1, 1, 2), (31, 3, 3), (33, 33, 7), (300, 64, 33), (129, 512, 64), (600, 16, 5)]   # (n_train, F, C); the last has three parts
TRACE = (1, 20, 200)


def problem(nt, f, c):
    n = nt + 2 * max(200, c * 8)          # validation and test sets of 200 rows or more: one row is at most 0.5 % of a set
    x, y = pm.blobs(n, f, c, 100 + nt)
    perm = np.random.RandomState(nt).permutation(n)
    nv = (n - nt) // 2
    w0, b0 = pm.init(1, c, f, nt)
    return x, y, perm[:nt], perm[nt:nt + nv], perm[nt + nv:], w0, b0


@pytest.mark.parametrize("select", ["scripts", "cca"])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("nt,f,c", SHAPES)
def test_mirror_against_the_float64_restatement(mirror, nt, f, c, wd, select):
    x, y, tr, va, te, w0, b0 = problem(nt, f, c)
    kw = dict(weight_decay=wd, test_interval=20, select=select, trace_epochs=TRACE)
    m = pm.run(mirror, x, y, tr, va, te, w0, b0, 200, trace=True, **kw)
    ref = pm.restatement(x, y, tr, va, te, w0[0], b0[0], 200, **kw)
    assert m["status"] == 0
    for j, ep in enumerate(TRACE):
        mw, rw = m["trace_w"][j, 0], ref["trace_w"][j]
        prel = np.abs(mw[:-1] - rw[:-1]).max() / np.abs(rw[:-1]).max()
        lrel = abs(mw[-1] - rw[-1]) / abs(rw[-1])
        print(f"n={nt} F={f} C={c} wd={wd} {select} epoch {ep}: parameters rel {prel:.3g}, loss {rw[-1]:.4g} rel {lrel:.3g}")
        assert prel <= PARAM_BOUND and lrel <= LOSS_BOUND
    # the logits of the last evaluation (epoch 199 is a scoring epoch of both rules) from the final parameters
    rows = np.concatenate([va, te])
    zm = x[rows].astype(np.float64) @ m["weight"][0].astype(np.float64).T + m["bias"][0].astype(np.float64)
    zr = np.concatenate(ref["logits"][-1])
    zdiff = np.abs(zm - zr).max()
    print(f"n={nt} F={f} C={c} wd={wd} {select}: logits abs {zdiff:.3g}")
    assert zdiff <= LOGIT_BOUND
    # the predictions of every evaluation; a row may be left out only where the restatement's own gap decides nothing
    assert len(ref["logits"]) == m["trace"].shape[0] == len(pm.scoring_epochs(200, 20, select))
    open_selection = False
    for e, (zv, zt) in enumerate(ref["logits"]):
        z = np.concatenate([zv, zt])
        top = np.sort(z, -1)
        loose = (top[:, -1] - top[:, -2]) < 4 * zdiff        # (four times the logit difference measured for this case, above)
        for part, lo in ((zv, 0), (zt, len(zv))):
            assert loose[lo:lo + len(part)].mean() <= 0.01
        open_selection |= bool(loose.any())
        assert np.array_equal(m["trace"][e][~loose], z.argmax(-1)[~loose]), f"evaluation {e}"
    if not open_selection:   # no left-out row could change the selection
        assert m["best_epoch"][0] == ref["best_epoch"] and m["best_val_correct"][0] == ref["best_val_correct"]
        assert m["micro_f1"][0] == ref["micro_f1"] and m["accuracy"][0] == ref["accuracy"]
        assert abs(m["macro_f1"][0] - ref["macro_f1"]) <= 4e-16      # (numpy's mean adds in pairs, the rule in label order)
        pt = np.concatenate(ref["logits"][ref["epochs"].index(ref["best_epoch"])]).argmax(-1) if m["best_val_correct"][0] > 0 else None
        if pt is not None:
            assert np.array_equal(m["confusion"][0, 0], pm.numpy_scores(y[va], pt[:len(va)], c)[3])
            assert np.array_equal(m["confusion"][0, 1], pm.numpy_scores(y[te], pt[len(va):], c)[3])


def test_expw_and_the_clamp(mirror):
    mirror.probe_expw.restype = ctypes.c_float
    mirror.probe_expw.argtypes = [ctypes.c_float]
    for v in (0.0, -1e-3, -1.0, -20.0, -80.0):
        assert abs(mirror.probe_expw(v) - np.exp(np.float64(np.float32(v)))) <= 2e-7 * np.exp(v)
    assert mirror.probe_expw(-80.0) > 1.1754944e-38       # a normal float32 at the clamp


# ------------------------------------------------------------------------------------------------ the scores
def score_case(mirror, y, pred_by_w, c):
    """A probe on one-hot features whose weights send row i to pred_by_w[i]: scores of the mirror on all rows."""
    n = len(y)
    x = np.eye(n, dtype=np.float32)
    w = np.zeros((1, c, n), dtype=np.float32)
    w[0, pred_by_w, np.arange(n)] = 1.0
    return pm.scores(mirror, x, y, np.arange(n), w, np.zeros((1, c), dtype=np.float32))


SCORE_CASES = {
    "a class absent from the true labels but predicted": ([0, 0, 1, 1, 0], [0, 2, 1, 2, 0], 3),
    "a class absent from both": ([0, 1, 1, 0, 3], [0, 1, 0, 0, 3], 5),
    "a single class": ([1, 1, 1], [1, 1, 1], 2),
    "nothing right": ([0, 1, 2], [1, 2, 0], 3),
    "many": (list(np.random.RandomState(1).randint(0, 7, 200)), list(np.random.RandomState(2).randint(0, 6, 200)), 8),
}


@pytest.mark.parametrize("name", sorted(SCORE_CASES))
def test_scores_against_numpy(mirror, name):
    y, p, c = SCORE_CASES[name]
    y, p = np.asarray(y, dtype=np.int64), np.asarray(p, dtype=np.int64)
    m = score_case(mirror, y, p, c)
    acc, micro, macro, conf = pm.numpy_scores(y, p, c)
    assert np.array_equal(m["pred"], p) and np.array_equal(m["confusion"][0], conf)
    assert m["accuracy"][0] == acc and m["micro_f1"][0] == micro and abs(m["macro_f1"][0] - macro) <= 2e-16


@pytest.mark.parametrize("name", sorted(SCORE_CASES))
def test_scores_against_sklearn(mirror, name):
    metrics = pytest.importorskip("sklearn.metrics")
    y, p, c = SCORE_CASES[name]
    m = score_case(mirror, np.asarray(y, dtype=np.int64), np.asarray(p, dtype=np.int64), c)
    assert m["accuracy"][0] == metrics.accuracy_score(y, p)
    assert abs(m["micro_f1"][0] - metrics.f1_score(y, p, average="micro")) <= 2e-16
    assert abs(m["macro_f1"][0] - metrics.f1_score(y, p, average="macro")) <= 2e-16


def test_ties_resolve_to_the_lowest_index(mirror):
    x, y = pm.blobs(60, 5, 4, 3)
    w, b = pm.init(1, 4, 5, 4)
    w[0, 3] = w[0, 1]; b[0, 3] = b[0, 1]                      # classes 1 and 3 tie everywhere
    m = pm.scores(mirror, x, y, np.arange(60), w, b)
    z = x.astype(np.float64) @ w[0].astype(np.float64).T + b[0]
    assert not (m["pred"] == 3).any() and (m["pred"] == 1).any()
    clear = np.sort(z[:, :3], -1)
    clear = (clear[:, -1] - clear[:, -2]) > 1e-4
    assert np.array_equal(m["pred"][clear], z[:, :3].argmax(-1)[clear])
    w[0, :] = 0.0; b[0, :] = 0.25
    assert (pm.scores(mirror, x, y, np.arange(60), w, b)["pred"] == 0).all()


# ------------------------------------------------------------------------------------------------ order and invariance
KEYS = ("weight", "bias", "micro_f1", "macro_f1", "accuracy", "loss", "best_epoch", "best_val_correct", "confusion")


def ragged(n, r, seed, nt=40):
    rng = np.random.RandomState(seed)
    perms = [rng.permutation(n) for _ in range(r)]
    return ([p[:nt + 5 * k] for k, p in enumerate(perms)], [p[nt + 5 * k:nt + 5 * k + 30 - k] for k, p in enumerate(perms)],
            [p[-(25 + 2 * k):] for k, p in enumerate(perms)])


def test_threads_and_tiling_change_no_bit(mirror):
    """The mirror computes every row's softmax and every element of dW on its own, so `block` and `threads` only change how they
    are dealt out: this pins the mirror, not the kernels.  The guard against an order that depends on the grid is the bit-for-bit
    comparison on the device (tests/test_gpu_probe.py: several parts, several runs)."""
    x, y = pm.blobs(700, 9, 4, 5)
    tr, va, te = ragged(700, 1, 6, nt=520)
    w0, b0 = pm.init(1, 4, 9, 7)
    base = pm.run(mirror, x, y, tr, va, te, w0, b0, 25, test_interval=5, block=32, threads=8)
    for block, threads in ((1, 8), (7, 3), (1000, 1)):
        other = pm.run(mirror, x, y, tr, va, te, w0, b0, 25, test_interval=5, block=block, threads=threads)
        for key in KEYS:
            assert base[key].tobytes() == other[key].tobytes(), (block, threads, key)


def test_parts_depend_on_the_shape_alone(mirror):
    for n in (1, 255, 256, 257, 512, 513, 2708, 16384, 16385, 169343):
        for f, c in ((1, 2), (512, 64)):
            p = mirror.probe_parts(n, f, c)
            assert p == min((n + 255) // 256, 64) and mirror.probe_part_begin(n, f, c, 0) == 0 and mirror.probe_part_begin(n, f, c, p) == n
            assert all(mirror.probe_part_begin(n, f, c, q) % 256 == 0 for q in range(p))
    assert [mirror.probe_class_pad(c) for c in (2, 8, 9, 16, 17, 33, 64)] == [8, 8, 16, 16, 32, 64, 64]


def test_runs_in_one_call_equal_single_calls_with_ragged_sets(mirror):
    x, y = pm.blobs(150, 6, 3, 8)
    tr, va, te = ragged(150, 3, 9)
    w0, b0 = pm.init(3, 3, 6, 10)
    both = pm.run(mirror, x, y, tr, va, te, w0, b0, 30, test_interval=5, weight_decay=1e-4)
    for k in range(3):
        one = pm.run(mirror, x, y, tr[k], va[k], te[k], w0[k:k + 1], b0[k:k + 1], 30, test_interval=5, weight_decay=1e-4)
        for key in KEYS:
            assert one[key].tobytes() == both[key][k:k + 1].tobytes(), (k, key)


def test_a_repeated_index_counts_twice(mirror):
    x, y = pm.blobs(80, 4, 3, 11)
    tr, va, te = np.arange(30), np.arange(30, 55), np.arange(55, 80)
    w0, b0 = pm.init(1, 3, 4, 12)
    twice = pm.run(mirror, x, y, np.concatenate([tr, [3, 3, 7]]), va, np.concatenate([te, [60]]), w0, b0, 10, test_interval=1)
    x2, y2 = np.concatenate([x, x[[3, 3, 7, 60]]]), np.concatenate([y, y[[3, 3, 7, 60]]])
    copy = pm.run(mirror, x2, y2, np.concatenate([tr, [80, 81, 82]]), va, np.concatenate([te, [83]]), w0, b0, 10, test_interval=1)
    for key in KEYS:
        assert twice[key].tobytes() == copy[key].tobytes(), key
    assert twice["confusion"][0, 1].sum() == 26
    assert pm.run(mirror, x, y, tr, va, te, w0, b0, 10, test_interval=1)["weight"].tobytes() != twice["weight"].tobytes()


def test_permuting_a_list_changes_bits_only_through_the_order(mirror):
    """The scores count rows, so the order of a validation or test list changes nothing; the order of the training list is the
    order of the gradient's chains, so it may change the last bits of the parameters and changes nothing else of size."""
    x, y = pm.blobs(120, 8, 3, 13)
    tr, va, te = np.arange(50), np.arange(50, 85), np.arange(85, 120)
    w0, b0 = pm.init(1, 3, 8, 14)
    base = pm.run(mirror, x, y, tr, va, te, w0, b0, 20, test_interval=5)
    other = pm.run(mirror, x, y, tr, va[::-1], te[::-1], w0, b0, 20, test_interval=5)
    for key in KEYS:
        assert base[key].tobytes() == other[key].tobytes(), key
    shuffled = pm.run(mirror, x, y, tr[::-1], va, te, w0, b0, 20, test_interval=5)
    assert np.abs(shuffled["weight"] - base["weight"]).max() <= 1e-4 * np.abs(base["weight"]).max()
    same_image = pm.run(mirror, x[::-1], y[::-1], 119 - tr, 119 - va, 119 - te, w0, b0, 20, test_interval=5)   # the rows moved, the lists' order kept
    for key in KEYS:
        assert base[key].tobytes() == same_image[key].tobytes(), key


def test_the_status_word_of_the_mirror(mirror):
    x, y = pm.blobs(40, 3, 3, 15)
    w0, b0 = pm.init(1, 3, 3, 16)
    a = np.arange(40)
    assert pm.run(mirror, x, y, a, a, a, w0, b0, 2)["status"] == 0
    bad = a.copy(); bad[4] = 40
    assert pm.run(mirror, x, y, a, bad, a, w0, b0, 2, test_interval=1)["status"] == 2
    assert pm.run(mirror, x, y, a, a, a, w0[:, :2], b0[:, :2], 2)["status"] == 3


# ------------------------------------------------------------------------------------------------ the index arithmetic, under the sanitizers
def test_the_index_arithmetic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "probe_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "rlap_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "csrc", "probe_main.cc")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), "600"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "600 sizes, 0 failures" in r.stdout


# ------------------------------------------------------------------------------------------------ the entry points on a stub
SIGS = {
    "rlap_linear_probe": "h x N F ldx y C R train train_ptr valid valid_ptr test test_ptr epochs lr wd interval select beta1 beta2 eps "
                         "w0 b0 w b scores best confusion status info",
    "rlap_probe_scores": "h x N F ldx y C R index ptr w b pred confusion scores status info",
}
ARENA = 4321


def f32_at(addr, count):
    return list(ctypes.cast(addr, ctypes.POINTER(ctypes.c_float))[:count])


class ProbeStub(StubLib):
    """Records both exports; writes scores r + 0.25 j, best (3, 4), status 0 and ones into the other results."""

    def __init__(self):
        super().__init__(SIGS)

    def export(self, name, a):
        R, C, F = a["R"], a["C"], a["F"]
        rec = {k: a[k] for k in a if k in ("N", "F", "ldx", "C", "R", "epochs", "lr", "wd", "interval", "select", "beta1", "beta2", "eps")}
        rec["x_first_row"] = f32_at(a["x"], F)
        rec["y"] = i64_at(a["y"], a["N"])
        train = name == "rlap_linear_probe"
        for key, p in ((("train", "train_ptr"), ("valid", "valid_ptr"), ("test", "test_ptr")) if train else (("index", "ptr"),)):
            rec[p] = list(a[p])
            rec[key] = i64_at(a[key], rec[p][-1])
        rec["w0"], rec["b0"] = f32_at(a["w0" if train else "w"], R * C * F), f32_at(a["b0" if train else "b"], R * C)
        self.calls.append((name, rec))
        if self.status:
            a["info"]._obj.detail = 2
            return self.status
        nsc = 4 if train else 3
        sc = ctypes.cast(a["scores"], ctypes.POINTER(ctypes.c_double))
        for r in range(R):
            for j in range(nsc):
                sc[r * nsc + j] = r + 0.25 * j
        ctypes.cast(a["status"], ctypes.POINTER(ctypes.c_int32))[0] = 0
        conf = ctypes.cast(a["confusion"], ctypes.POINTER(ctypes.c_int64))
        for i in range(R * (2 if train else 1) * C * C):
            conf[i] = 1
        if train:
            best = ctypes.cast(a["best"], ctypes.POINTER(ctypes.c_int64))
            for r in range(R):
                best[2 * r], best[2 * r + 1] = 3, 4
            for key, count in (("w", R * C * F), ("b", R * C)):
                out = ctypes.cast(a[key], ctypes.POINTER(ctypes.c_float))
                for i in range(count):
                    out[i] = 1.0
        else:
            pred = ctypes.cast(a["pred"], ctypes.POINTER(ctypes.c_int64))
            for i in range(rec["ptr"][-1]):
                pred[i] = 1
        info = a["info"]._obj
        info.runs, info.parts, info.launches, info.arena_bytes, info.host_syncs, info.detail = R, 2, 9, ARENA, 0, 0
        return 0


@pytest.fixture
def lib(monkeypatch):
    return stub_ops(monkeypatch, ProbeStub())


def data(n=12, f=3, c=3):
    x = torch.arange(n * f, dtype=torch.float32).reshape(n, f) / 4.0
    return x, torch.arange(n) % c


def test_arguments_of_linear_probe(lib):
    x, y = data()
    tr, va, te = [torch.tensor([0, 1, 2]), torch.tensor([5, 4, 3, 3])], [torch.tensor([6]), torch.tensor([7, 8])], [torch.tensor([9, 10]), torch.tensor([11])]
    w, b = torch.full((2, 3, 3), 0.5), torch.full((2, 3), -0.5)
    res = ops.linear_probe(x, y, tr, va, te, epochs=7, lr=0.02, weight_decay=1e-4, test_interval=3, select="cca", weight=w, bias=b,
                           betas=(0.8, 0.9), eps=1e-6)
    (name, c), = lib.exports()
    assert name == "rlap_linear_probe"
    assert (c["N"], c["F"], c["ldx"], c["C"], c["R"]) == (12, 3, 3, 3, 2)                     # C = y.max() + 1
    assert (c["epochs"], c["lr"], c["wd"], c["interval"], c["select"], c["beta1"], c["beta2"], c["eps"]) == (7, 0.02, 1e-4, 3, 1, 0.8, 0.9, 1e-6)
    assert c["train"] == [0, 1, 2, 5, 4, 3, 3] and c["train_ptr"] == [0, 3, 7] and c["valid"] == [6, 7, 8] and c["valid_ptr"] == [0, 1, 3]
    assert c["test"] == [9, 10, 11] and c["test_ptr"] == [0, 2, 3] and c["y"] == y.tolist() and c["x_first_row"] == x[0].tolist()
    assert c["w0"] == [0.5] * 18 and c["b0"] == [-0.5] * 6
    assert res["micro_f1"].tolist() == [0.0, 1.0] and res["macro_f1"].tolist() == [0.25, 1.25] and res["accuracy"].tolist() == [0.5, 1.5]
    assert res["loss"].tolist() == [0.75, 1.75] and res["best_epoch"].tolist() == [3, 3] and res["best_val_correct"].tolist() == [4, 4]
    assert res["confusion"].shape == (2, 2, 3, 3) and res["weight"].shape == (2, 3, 3) and res["bias"].shape == (2, 3) and int(res["status"]) == 0
    assert all(res[k].dtype == torch.float64 for k in ("micro_f1", "macro_f1", "accuracy", "loss")) and res["confusion"].dtype == torch.int64
    assert ops.last_stats == {"runs": 2, "parts": 2, "launches": 9, "arena_bytes": ARENA, "host_syncs": 0, "detail": 0}


def test_defaults_forms_of_the_sets_and_drawn_parameters(lib):
    x, y = data()
    gen = torch.Generator().manual_seed(3)
    ops.linear_probe(x, y, torch.tensor([0, 1]), (torch.tensor([2, 3, 4]), [0, 3]), (torch.tensor([5, 6]), torch.tensor([0, 2])), num_classes=5,
                     generator=gen)
    (_, c), = lib.exports()
    assert (c["C"], c["R"], c["epochs"], c["lr"], c["wd"], c["interval"], c["select"], c["beta1"], c["beta2"], c["eps"]) == \
        (5, 1, 2000, 0.01, 0.0, 20, 0, 0.9, 0.999, 1e-8)
    assert c["train_ptr"] == [0, 2] and c["valid"] == [2, 3, 4] and c["test_ptr"] == [0, 2]
    w, b = ops.probe_init(1, 5, 3, torch.Generator().manual_seed(3))
    assert c["w0"] == w.reshape(-1).tolist() and c["b0"] == b.reshape(-1).tolist()
    # the draws are the reference's: nn.Linear's defaults, then xavier_uniform_ on the weight, from the global generator
    torch.manual_seed(3)
    fc = torch.nn.Linear(3, 5)
    torch.nn.init.xavier_uniform_(fc.weight.data)
    assert torch.equal(fc.weight.data, w[0]) and torch.equal(fc.bias.data, b[0])


def test_a_strided_view_is_passed_in_place_and_others_are_packed(lib):
    x, y = data(12, 6)
    idx = torch.arange(12)
    ops.linear_probe(x[:, 1:4], y, idx, idx, idx, epochs=1)
    ops.linear_probe(x.t()[:6, :].t()[:, ::2], y, idx, idx, idx, epochs=1)
    (_, a), (_, b) = lib.exports()
    assert (a["F"], a["ldx"]) == (3, 6) and a["x_first_row"] == x[0, 1:4].tolist()
    assert (b["F"], b["ldx"]) == (3, 3) and b["x_first_row"] == x[0, ::2].tolist()


def test_arguments_of_probe_scores(lib):
    x, y = data()
    res = ops.probe_scores(x, y, [torch.tensor([3, 1]), torch.tensor([2])], torch.full((2, 4, 3), 2.0), torch.zeros(2, 4))
    (name, c), = lib.exports()
    assert name == "rlap_probe_scores" and (c["N"], c["F"], c["C"], c["R"]) == (12, 3, 4, 2) and c["index"] == [3, 1, 2] and c["ptr"] == [0, 2, 3]
    assert res["pred"].tolist() == [1, 1, 1] and res["confusion"].shape == (2, 4, 4) and res["macro_f1"].tolist() == [0.25, 1.25]
    ops.probe_scores(x, y, torch.tensor([0]), torch.zeros(3, 3), torch.zeros(3))     # one run without the leading axis
    assert lib.exports()[1][1]["R"] == 1


def test_a_refusal_of_the_library_raises(lib):
    x, y = data()
    lib.status = 3
    with pytest.raises(ValueError, match="detail 2"):
        ops.linear_probe(x, y, torch.tensor([0]), torch.tensor([1]), torch.tensor([2]), epochs=1)
    lib.status = 9
    with pytest.raises(RuntimeError):
        ops.linear_probe(x, y, torch.tensor([0]), torch.tensor([1]), torch.tensor([2]), epochs=1)


I = torch.tensor([0, 1])
BAD = [
    dict(x=torch.zeros(4, 3, dtype=torch.float64)), dict(x=torch.zeros(4)), dict(x=torch.zeros(4, 513)), dict(x=torch.zeros(4, 0)),
    dict(y=torch.zeros(4, dtype=torch.int32)), dict(y=torch.zeros(5, dtype=torch.int64)), dict(num_classes=1), dict(num_classes=65),
    dict(y=torch.zeros(4, dtype=torch.int64)),                                     # y.max() + 1 = 1 class
    dict(train=torch.tensor([], dtype=torch.int64)), dict(valid=[I, torch.tensor([], dtype=torch.int64)], train=[I, I], test=[I, I]),
    dict(train=[I, I]), dict(train=torch.tensor([0.0, 1.0])), dict(train=(I, [0, 1])), dict(train=(I, [1, 2])), dict(train="all"),
    dict(test=torch.zeros((2, 1), dtype=torch.int64)), dict(train=[I] * 33, valid=[I] * 33, test=[I] * 33),
    dict(lr=float("nan")), dict(lr=float("inf")), dict(weight_decay=-1.0), dict(betas=(1.0, 0.9)), dict(eps=0.0), dict(epochs=0),
    dict(test_interval=0), dict(select="sklearn"), dict(weight=torch.zeros(1, 3, 3)), dict(weight=torch.zeros(1, 2, 3), bias=torch.zeros(1, 3)),
    dict(weight=torch.zeros(1, 3, 3, dtype=torch.float64), bias=torch.zeros(1, 3)), dict(weight=torch.zeros(1, 3, 3), bias=torch.zeros(3)),
]


@pytest.mark.parametrize("over", BAD, ids=[",".join(sorted(o)) + str(k) for k, o in enumerate(BAD)])
def test_bad_arguments_raise_value_error_before_any_call(lib, monkeypatch, over):
    def reached(*args, **kw):
        raise AssertionError("the device or the library was reached")
    monkeypatch.setattr(ops, "_device_for", reached)
    monkeypatch.setattr(ops, "_handle_obj", reached)
    kw = dict(x=torch.zeros(4, 3), y=torch.tensor([0, 1, 2, 0]), train=I, valid=I, test=I, num_classes=None)
    kw.update(over)
    with pytest.raises(ValueError):
        ops.linear_probe(kw.pop("x"), kw.pop("y"), kw.pop("train"), kw.pop("valid"), kw.pop("test"), **kw)
    with pytest.raises(ValueError):
        ops.probe_scores(torch.zeros(4, 3), torch.tensor([0, 1, 2, 0]), torch.tensor([], dtype=torch.int64), torch.zeros(1, 3, 3), torch.zeros(1, 3))
    assert lib.exports() == []


def test_layout_of_the_info_structure(tmp_path):
    layout_matches_the_header(tmp_path, "rlap_probe_info", "ProbeInfo")
    assert (_lib.PROBE_SELECT_SCRIPTS, _lib.PROBE_SELECT_CCA) == (0, 1)
    hdr = open(os.path.join(ROOT, "include", "rlap_hip.h")).read()
    assert "RLAP_PROBE_SELECT_SCRIPTS = 0, RLAP_PROBE_SELECT_CCA = 1" in hdr


# ------------------------------------------------------------------------------------------------ the adapters
def test_get_split_sizes_disjointness_and_runs():
    s = adapters.get_split(103, generator=torch.Generator().manual_seed(1))
    assert {k: len(v) for k, v in s.items()} == {"train": 10, "valid": 82, "test": 11}    # as published: 'valid' takes test_size rows
    assert sorted(torch.cat(list(s.values())).tolist()) == list(range(103))
    s = adapters.get_split(50, train_ratio=0.2, test_ratio=0.5)
    assert {k: len(v) for k, v in s.items()} == {"train": 10, "valid": 25, "test": 15}
    runs = adapters.get_split(40, runs=3, generator=torch.Generator().manual_seed(2))
    assert len(runs) == 3 and all(sorted(torch.cat(list(r.values())).tolist()) == list(range(40)) for r in runs)
    assert not torch.equal(runs[0]["train"], runs[1]["train"])
    torch.manual_seed(7)
    a = adapters.get_split(30)
    torch.manual_seed(7)
    assert torch.equal(torch.randperm(30)[:3], a["train"])
    with pytest.raises(AssertionError):
        adapters.get_split(10, 0.5, 0.5)


def test_lr_evaluator_makes_one_call_and_returns_python_floats(lib):
    x, y = data()
    splits = adapters.get_split(12, 0.25, 0.5, runs=2, generator=torch.Generator().manual_seed(4))
    ev = adapters.LREvaluator(num_epochs=9, learning_rate=0.05, weight_decay=1e-4, test_interval=3, generator=torch.Generator().manual_seed(5))
    out = ev.evaluate_runs(x, y, splits)
    (name, c), = lib.exports()
    assert (c["R"], c["epochs"], c["lr"], c["wd"], c["interval"], c["select"]) == (2, 9, 0.05, 1e-4, 3, 0)
    assert c["train"] == splits[0]["train"].tolist() + splits[1]["train"].tolist() and c["test_ptr"] == [0, 3, 6]
    assert out == [{"micro_f1": 0.0, "macro_f1": 0.25, "accuracy": 0.5}, {"micro_f1": 1.0, "macro_f1": 1.25, "accuracy": 1.5}]
    assert all(type(v) is float for d in out for v in d.values())
    one = adapters.LREvaluator(num_epochs=2, select="cca")(x, y, splits[0])
    assert one == out[0] and lib.exports()[1][1]["select"] == 1 and lib.exports()[1][1]["R"] == 1
