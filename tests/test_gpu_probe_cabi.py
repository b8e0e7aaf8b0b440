"""rlap_linear_probe and rlap_probe_scores called through the C ABI on raw device pointers and a handle of the test's own, after the
pattern of tests/test_gpu_g2l_cabi.py: one good call of each against ops; the statuses of the host checks, which answer before
anything is launched (the result buffers are filled with a pattern first and must come back unchanged); the status word the kernels
raise for a label and for an index out of range."""
import ctypes

import numpy as np
import pytest
import torch

import probe_mirror as pm

pytestmark = pytest.mark.gpu

OK, INDEX_RANGE, BAD_ARG, TOO_LARGE = 0, 2, 3, 9
PATTERN = -7


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rlap_amd import _lib
    return {"lib": _lib.load(), "_lib": _lib}


@pytest.fixture
def handle(env):
    h = ctypes.c_void_p()
    assert env["lib"].rlap_create(ctypes.byref(h)) == 0
    yield h
    torch.cuda.synchronize()
    assert env["lib"].rlap_destroy(h) == 0


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def host(values):
    return (ctypes.c_int64 * len(values))(*values)


def inputs(n=90, f=9, c=4, r=2):
    x, y = pm.blobs(n, f, c, 61)
    rng = np.random.RandomState(62)
    lists = {k: [rng.permutation(n)[:m + j] for j in range(r)] for k, m in (("train", 40), ("valid", 20), ("test", 25))}
    w0, b0 = pm.init(r, c, f, 63)
    return x, y, lists, w0, b0


def call(env, h, x, y, lists, w0, b0, c, over=None, epochs=10):
    """rlap_linear_probe: (status, the result buffers, the info).  `over` replaces arguments by name."""
    n, f = x.shape
    r = b0.shape[0]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = {k: dev(np.concatenate(v)) for k, v in lists.items()}
    ptrs = {k: [0] + list(np.cumsum([len(a) for a in v])) for k, v in lists.items()}
    keep.update(x=dev(x), y=dev(y), w0=dev(w0), b0=dev(b0))
    out = {"w": torch.full((r, c, f), float(PATTERN), device="cuda"), "b": torch.full((r, c), float(PATTERN), device="cuda"),
           "scores": torch.full((r, 4), float(PATTERN), dtype=torch.float64, device="cuda"),
           "best": torch.full((r, 2), PATTERN, dtype=torch.int64, device="cuda"),
           "confusion": torch.full((r, 2, c, c), PATTERN, dtype=torch.int64, device="cuda"),
           "status": torch.full((1,), PATTERN, dtype=torch.int32, device="cuda")}
    a = {"x": ptr(keep["x"]), "N": n, "F": f, "ldx": f, "y": ptr(keep["y"]), "C": c, "R": r,
         "train": ptr(keep["train"]), "train_ptr": host(ptrs["train"]), "valid": ptr(keep["valid"]), "valid_ptr": host(ptrs["valid"]),
         "test": ptr(keep["test"]), "test_ptr": host(ptrs["test"]), "epochs": epochs, "lr": 0.01, "wd": 0.0, "interval": 5, "select": 0,
         "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "w0": ptr(keep["w0"]), "b0": ptr(keep["b0"])}
    a.update({k: ptr(v) for k, v in out.items()})
    a.update(over or {})
    info = env["_lib"].ProbeInfo()
    rc = env["lib"].rlap_linear_probe(h, a["x"], a["N"], a["F"], a["ldx"], a["y"], a["C"], a["R"], a["train"], a["train_ptr"], a["valid"],
                                      a["valid_ptr"], a["test"], a["test_ptr"], a["epochs"], a["lr"], a["wd"], a["interval"], a["select"],
                                      a["beta1"], a["beta2"], a["eps"], a["w0"], a["b0"], a["w"], a["b"], a["scores"], a["best"],
                                      a["confusion"], a["status"], ctypes.byref(info))
    torch.cuda.synchronize()
    return rc, out, info


def untouched(out):
    return all(bool((t == PATTERN).all()) for t in out.values())


def test_a_good_call_equals_ops(env, handle):
    from rlap_amd import ops
    x, y, lists, w0, b0 = inputs()
    rc, out, info = call(env, handle, x, y, lists, w0, b0, 4)
    assert rc == OK and int(out["status"]) == OK
    assert (info.runs, info.parts, info.host_syncs, info.detail) == (2, 1, 0, 0) and info.launches == 2 + 2 * 10 + 2 * 2 + 2 and info.arena_bytes > 0
    t = lambda k: [torch.from_numpy(a).cuda() for a in lists[k]]
    res = ops.linear_probe(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), t("train"), t("valid"), t("test"), num_classes=4, epochs=10,
                           test_interval=5, weight=torch.from_numpy(w0), bias=torch.from_numpy(b0))
    assert torch.equal(out["w"], res["weight"]) and torch.equal(out["b"], res["bias"]) and torch.equal(out["confusion"], res["confusion"])
    assert torch.equal(out["scores"][:, 0], res["micro_f1"]) and torch.equal(out["best"][:, 1], res["best_val_correct"])


def test_the_host_checks_answer_before_anything_is_launched(env, handle):
    x, y, lists, w0, b0 = inputs()
    empty = host([0, 0, 41])
    cases = [({"F": 513, "ldx": 513}, TOO_LARGE, 1), ({"C": 65}, TOO_LARGE, 1), ({"C": 1}, BAD_ARG, 1), ({"F": 0}, BAD_ARG, 1),
             ({"ldx": 8}, BAD_ARG, 1), ({"R": 33}, TOO_LARGE, 1), ({"valid_ptr": empty}, BAD_ARG, 2), ({"train_ptr": host([1, 40, 81])}, BAD_ARG, 2),
             ({"lr": float("nan")}, BAD_ARG, 3), ({"lr": float("inf")}, BAD_ARG, 3), ({"epochs": 0}, BAD_ARG, 3), ({"select": 2}, BAD_ARG, 3),
             ({"x": None}, BAD_ARG, 4), ({"status": None}, BAD_ARG, 4)]
    for over, want, detail in cases:
        rc, out, info = call(env, handle, x, y, lists, w0, b0, 4, over=over)
        assert (rc, info.detail) == (want, detail), (over, rc, info.detail)
        assert untouched(out), over


def test_a_label_and_an_index_out_of_range_raise_the_status_word(env, handle):
    x, y, lists, w0, b0 = inputs()
    rc, out, _ = call(env, handle, x, y, lists, w0, b0, 3, epochs=2)     # the labels reach 3 with three classes
    assert rc == OK and int(out["status"]) == BAD_ARG
    bad = {k: [a.copy() for a in v] for k, v in lists.items()}
    bad["test"][1][3] = -1
    rc, out, _ = call(env, handle, x, y, bad, w0, b0, 4, epochs=2)
    assert rc == OK and int(out["status"]) == OK                        # (no evaluation in two epochs: the test list is never read)
    rc, out, _ = call(env, handle, x, y, bad, w0, b0, 4, epochs=2, over={"interval": 1})
    assert rc == OK and int(out["status"]) == INDEX_RANGE
    bad["train"][0][0] = x.shape[0]
    rc, out, _ = call(env, handle, x, y, bad, w0, b0, 4, epochs=2)
    assert rc == OK and int(out["status"]) == INDEX_RANGE and bool(torch.isfinite(out["w"]).all())


def test_probe_scores_through_the_abi(env, handle):
    from rlap_amd import ops
    x, y, lists, w0, b0 = inputs()
    n, f = x.shape
    idx = np.concatenate(lists["test"])
    p = [0] + list(np.cumsum([len(a) for a in lists["test"]]))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    keep = [dev(x), dev(y), dev(idx), dev(w0), dev(b0)]
    pred = torch.full((len(idx),), PATTERN, dtype=torch.int64, device="cuda")
    conf = torch.full((2, 4, 4), PATTERN, dtype=torch.int64, device="cuda")
    scores = torch.full((2, 3), float(PATTERN), dtype=torch.float64, device="cuda")
    status = torch.full((1,), PATTERN, dtype=torch.int32, device="cuda")
    info = env["_lib"].ProbeInfo()
    args = lambda C, hp: (handle, ptr(keep[0]), n, f, f, ptr(keep[1]), C, 2, ptr(keep[2]), hp, ptr(keep[3]), ptr(keep[4]), ptr(pred), ptr(conf),
                          ptr(scores), ptr(status), ctypes.byref(info))
    assert env["lib"].rlap_probe_scores(*args(65, host(p))) == TOO_LARGE and env["lib"].rlap_probe_scores(*args(4, host([0, 0, 5]))) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((pred == PATTERN).all()) and bool((conf == PATTERN).all())
    assert env["lib"].rlap_probe_scores(*args(4, host(p))) == OK
    torch.cuda.synchronize()
    res = ops.probe_scores(keep[0], keep[1], [dev(a) for a in lists["test"]], keep[3], keep[4])
    assert int(status) == OK and info.launches == 3
    assert torch.equal(pred, res["pred"]) and torch.equal(conf, res["confusion"]) and torch.equal(scores[:, 1], res["macro_f1"])
