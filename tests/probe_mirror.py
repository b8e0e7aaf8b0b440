"""Loader of the linear-probe evaluator's host mirror (tests/csrc/probe_mirror.cc around rlap_amd/csrc/rlap_probe.h), the inputs
and the float64 torch restatements of the reference's loops (scripts/node_shared.py:163-230, CCA-SSG/main.py:152-194), shared by
tests/test_probe_cpu.py and the GPU tests."""
import ctypes
import os
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_probe.h")
SRC = os.path.join(ROOT, "tests", "csrc", "probe_mirror.cc")
THREADS = 8
SELECT = {"scripts": 0, "cca": 1}


def build(directory):
    """Compiles the mirror into `directory` (contraction off, as the library) and declares its prototypes."""
    so = os.path.join(str(directory), "libprobe_mirror.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-I", os.path.dirname(HDR), "-o", so, SRC])
    lib = ctypes.CDLL(so)
    dbl, i64, ci, vp = ctypes.c_double, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    lib.probe_parts.restype = i64
    lib.probe_parts.argtypes = [i64, i64, i64]
    lib.probe_part_begin.restype = i64
    lib.probe_part_begin.argtypes = [i64, i64, i64, i64]
    lib.probe_class_pad.restype = i64
    lib.probe_class_pad.argtypes = [i64]
    lib.probe_scores_of.restype = None
    lib.probe_scores_of.argtypes = [vp, i64, i64, vp]
    lib.probe_mirror_scores.restype = ci
    lib.probe_mirror_scores.argtypes = [vp, i64, i64, i64, vp, i64, i64, vp, vp, vp, vp, i64, ci, vp, vp, vp]
    lib.probe_mirror.restype = ci
    lib.probe_mirror.argtypes = [vp, i64, i64, i64, vp, i64, i64, vp, vp, vp, vp, vp, vp, i64, dbl, dbl, i64, ci, dbl, dbl, dbl, vp, vp,
                                 i64, ci, vp, vp, vp, vp, vp, vp, vp, i64, vp]
    return lib


def _lists(arg):
    """(concatenated int64 indices, [R+1] int64 offsets) of an index array or a list of them."""
    lists = [np.asarray(arg, dtype=np.int64)] if not isinstance(arg, (list, tuple)) else [np.asarray(a, dtype=np.int64) for a in arg]
    ptr = np.zeros(len(lists) + 1, dtype=np.int64)
    ptr[1:] = np.cumsum([len(a) for a in lists])
    return np.ascontiguousarray(np.concatenate(lists)), ptr


def scoring_epochs(epochs, test_interval, select):
    return [e for e in range(epochs) if select == "cca" or (e + 1) % test_interval == 0]


def run(lib, x, y, train, valid, test, w0, b0, epochs, lr=0.01, weight_decay=0.0, test_interval=20, select="scripts",
        betas=(0.9, 0.999), eps=1e-8, block=32, threads=THREADS, trace=False, trace_epochs=()):
    """The mirror on numpy inputs; the sets are index arrays or lists of them (runs).  Returns the call's results as a dict of
    arrays, with `trace` the predictions of every scoring evaluation ([evaluations][all validation rows | all test rows]) and with
    `trace_epochs` (counted from 1) the parameters and the loss after those epochs ([len][R][C F + C + 1])."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 2 and x.strides[1] == 4 and x.strides[0] % 4 == 0
    n, f = x.shape
    y = np.ascontiguousarray(y, dtype=np.int64)
    w0 = np.ascontiguousarray(w0, dtype=np.float32)
    b0 = np.ascontiguousarray(b0, dtype=np.float32)
    r, c = b0.shape
    assert w0.shape == (r, c, f)
    (tr, trp), (va, vap), (te, tep) = _lists(train), _lists(valid), _lists(test)
    assert len(trp) == len(vap) == len(tep) == r + 1
    w, b = np.empty_like(w0), np.empty_like(b0)
    scores, best, conf = np.empty((r, 4)), np.empty((r, 2), dtype=np.int64), np.empty((r, 2, c, c), dtype=np.int64)
    evals = len(scoring_epochs(epochs, test_interval, select))
    tbuf = np.full((evals, int(vap[-1] + tep[-1])), -1, dtype=np.int64) if trace else None
    tep_ = np.ascontiguousarray(trace_epochs, dtype=np.int64)
    tw = np.empty((len(tep_), r, c * f + c + 1)) if len(tep_) else None
    status = lib.probe_mirror(x.ctypes.data, n, f, x.strides[0] // 4, y.ctypes.data, c, r, tr.ctypes.data, trp.ctypes.data, va.ctypes.data,
                              vap.ctypes.data, te.ctypes.data, tep.ctypes.data, int(epochs), float(lr), float(weight_decay),
                              int(test_interval), SELECT[select], float(betas[0]), float(betas[1]), float(eps), w0.ctypes.data,
                              b0.ctypes.data, int(block), int(threads), w.ctypes.data, b.ctypes.data, scores.ctypes.data, best.ctypes.data,
                              conf.ctypes.data, tbuf.ctypes.data if trace else None, tep_.ctypes.data if len(tep_) else None, len(tep_),
                              tw.ctypes.data if len(tep_) else None)
    return {"weight": w, "bias": b, "micro_f1": scores[:, 0].copy(), "macro_f1": scores[:, 1].copy(), "accuracy": scores[:, 2].copy(),
            "loss": scores[:, 3].copy(), "best_epoch": best[:, 0].copy(), "best_val_correct": best[:, 1].copy(), "confusion": conf,
            "status": status, "trace": tbuf, "trace_w": tw, "valid_rows": int(vap[-1])}


def scores(lib, x, y, index, w, b, block=32, threads=THREADS):
    """The scoring pass alone: pred, confusion (R, C, C), micro_f1, macro_f1, accuracy, status."""
    x = np.asarray(x, dtype=np.float32)
    n, f = x.shape
    y = np.ascontiguousarray(y, dtype=np.int64)
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    r, c = b.shape
    idx, ptr = _lists(index)
    pred, conf, sc = np.empty(len(idx), dtype=np.int64), np.empty((r, c, c), dtype=np.int64), np.empty((r, 3))
    status = lib.probe_mirror_scores(x.ctypes.data, n, f, x.strides[0] // 4, y.ctypes.data, c, r, idx.ctypes.data, ptr.ctypes.data,
                                     w.ctypes.data, b.ctypes.data, int(block), int(threads), pred.ctypes.data, conf.ctypes.data, sc.ctypes.data)
    return {"pred": pred, "confusion": conf, "micro_f1": sc[:, 0].copy(), "macro_f1": sc[:, 1].copy(), "accuracy": sc[:, 2].copy(),
            "status": status}


# ---- inputs
def blobs(n, f, c, seed, sep=3.0):
    """Class-separated Gaussian blobs with moderate overlap: (x float32 (n, f), y int64 (n,)), every class present when n >= c."""
    rng = np.random.RandomState(seed)
    centres = rng.standard_normal((c, f)) * sep / np.sqrt(max(f, 1)) * 2.0
    y = np.arange(n) % c
    rng.shuffle(y)
    x = centres[y] + rng.standard_normal((n, f))
    return x.astype(np.float32), y.astype(np.int64)


def init(r, c, f, seed):
    """Initial parameters as the reference draws them (ops.probe_init), seeded."""
    from rlap_amd import ops
    w, b = ops.probe_init(r, c, f, torch.Generator().manual_seed(seed))
    return w.numpy(), b.numpy()


def numpy_scores(y_true, y_pred, c):
    """(accuracy, micro_f1, macro_f1, confusion) as sklearn's accuracy_score / f1_score compute them, in numpy."""
    conf = np.zeros((c, c), dtype=np.int64)
    np.add.at(conf, (y_true, y_pred), 1)
    tp = np.diag(conf).astype(np.float64)
    rs, cs = conf.sum(1), conf.sum(0)
    present = (rs + cs) > 0
    f1 = 2 * tp[present] / (rs + cs)[present]
    acc = tp.sum() / len(y_true)
    return acc, acc, float(f1.mean()), conf


# ---- the reference's loops, restated in float64 torch
def restatement(x, y, train, valid, test, w0, b0, epochs, lr=0.01, weight_decay=0.0, test_interval=20, select="scripts",
                trace_epochs=()):
    """One run of LREvaluator's loop (select="scripts") or CCA-SSG/main.py's (select="cca") in float64 with torch.optim.Adam on the
    CPU, from the given initial parameters.  Returns the selected scores, and per scoring evaluation the logits of the validation
    and test rows (for the tie margins), and the parameters and the loss after `trace_epochs`."""
    xt = torch.from_numpy(np.asarray(x, dtype=np.float32)).double()
    yt = torch.from_numpy(np.asarray(y, dtype=np.int64))
    tr, va, te = (torch.from_numpy(np.asarray(a, dtype=np.int64)) for a in (train, valid, test))
    c = b0.shape[0]
    fc = torch.nn.Linear(xt.shape[1], c).double()
    with torch.no_grad():
        fc.weight.copy_(torch.from_numpy(w0).double())
        fc.bias.copy_(torch.from_numpy(b0).double())
    opt = torch.optim.Adam(fc.parameters(), lr=lr, weight_decay=weight_decay)
    out = {"logits": [], "trace_w": [], "epochs": []}
    best_val, best_test, rec = 0, 0, {"micro_f1": 0.0, "macro_f1": 0.0, "accuracy": 0.0, "best_epoch": 0}
    for epoch in range(epochs):
        opt.zero_grad()
        loss = torch.nn.functional.nll_loss(torch.log_softmax(fc(xt[tr]), dim=-1), yt[tr])
        loss.backward()
        opt.step()
        if epoch + 1 in trace_epochs:
            out["trace_w"].append(np.concatenate([fc.weight.detach().numpy().ravel(), fc.bias.detach().numpy(), [float(loss.detach())]]))
        if select == "cca" or (epoch + 1) % test_interval == 0:
            with torch.no_grad():
                zv, zt = fc(xt[va]).numpy(), fc(xt[te]).numpy()
            out["logits"].append((zv, zt))
            out["epochs"].append(epoch)
            pv, pt = zv.argmax(-1), zt.argmax(-1)
            val, tst = int((pv == yt[va].numpy()).sum()), int((pt == yt[te].numpy()).sum())
            take = False
            if select == "cca":
                if val >= best_val:
                    best_val = val
                    if tst > best_test:
                        best_test, take = tst, True
            elif val > best_val:
                best_val, take = val, True
            if take:
                acc, micro, macro, _ = numpy_scores(yt[te].numpy(), pt, c)
                rec = {"micro_f1": micro, "macro_f1": macro, "accuracy": acc, "best_epoch": epoch}
    out.update(rec)
    out["best_val_correct"] = best_val
    return out
