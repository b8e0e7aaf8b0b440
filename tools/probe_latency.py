"""ops.linear_probe against a torch restatement of the reference's evaluators on the same tensors and the same device.
The baseline is LREvaluator's loop as published (scripts/node_shared.py:163-230): a Linear(F, C) under Adam, log-softmax + NLL,
and every test_interval epochs the test and validation predictions copied to the host for sklearn's accuracy_score / f1_score --
the host round trips are kept, they are what the call removes --, run once per split, one after the other, as test() does.  A
second baseline restates CCA-SSG/main.py:152-194's loop (evaluation every epoch, one host comparison an epoch).  Medians of 5
after a warm-up, host clock around a synchronise; the five times are printed too.  Prints one JSON line per shape and R (and appends
it to --out).  It also checks that two calls return equal bits.

  cora     : 2,708 rows, F = 256, C = 7        arxiv : 169,343 rows, F = 256, C = 40
  cs       : 34,493 rows, F = 256, C = 15      graph : 1,113 rows, F = 160, C = 2 (a graph-level shape)
    python tools/probe_latency.py
    python tools/probe_latency.py --shapes cora --runs 10 --no-torch      # the call alone (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rlap_amd import adapters, ops  # noqa: E402

SHAPES = {"cora": (2708, 256, 7), "cs": (34493, 256, 15), "arxiv": (169343, 256, 40), "graph": (1113, 160, 2)}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), [round(t, 2) for t in ts], res


def blobs(n, f, c, seed):
    gen = torch.Generator().manual_seed(seed)
    y = torch.randint(0, c, (n,), generator=gen)
    centres = torch.randn(c, f, generator=gen) * (4.0 / f ** 0.5)
    return (centres[y] + torch.randn(n, f, generator=gen)).cuda(), y.cuda()


def host_scores():
    try:
        from sklearn.metrics import accuracy_score, f1_score
        return "sklearn", accuracy_score, lambda a, b, average: f1_score(a, b, average=average)
    except ImportError:   # numpy's counts stand in: the round trips to the host stay
        import numpy as np

        def f1(a, b, average):
            if average == "micro":
                return float((a == b).mean())
            labels = np.union1d(a, b)
            return float(np.mean([2 * ((a == k) & (b == k)).sum() / ((a == k).sum() + (b == k).sum()) for k in labels]))
        return "numpy", lambda a, b: float((a == b).mean()), f1


def torch_lr_evaluator(x, y, split, w0, b0, epochs, interval, acc_fn, f1_fn):
    fc = torch.nn.Linear(x.shape[1], w0.shape[0]).cuda()
    with torch.no_grad():
        fc.weight.copy_(w0)
        fc.bias.copy_(b0)
    opt = torch.optim.Adam(fc.parameters(), lr=0.01, weight_decay=0.0)
    out_fn, crit = torch.nn.LogSoftmax(dim=-1), torch.nn.NLLLoss()
    best = {"val": 0, "micro_f1": 0, "macro_f1": 0, "accuracy": 0}
    for epoch in range(epochs):
        opt.zero_grad()
        loss = crit(out_fn(fc(x[split["train"]])), y[split["train"]])
        loss.backward()
        opt.step()
        if (epoch + 1) % interval == 0:
            y_test = y[split["test"]].detach().cpu().numpy()
            y_pred = fc(x[split["test"]]).argmax(-1).detach().cpu().numpy()
            acc, micro, macro = acc_fn(y_test, y_pred), f1_fn(y_test, y_pred, average="micro"), f1_fn(y_test, y_pred, average="macro")
            y_val = y[split["valid"]].detach().cpu().numpy()
            val = f1_fn(y_val, fc(x[split["valid"]]).argmax(-1).detach().cpu().numpy(), average="micro")
            if val > best["val"]:
                best = {"val": val, "micro_f1": micro, "macro_f1": macro, "accuracy": acc}
    return best


def torch_cca_loop(x, y, split, w0, b0, epochs):
    fc = torch.nn.Linear(x.shape[1], w0.shape[0]).cuda()
    with torch.no_grad():
        fc.weight.copy_(w0)
        fc.bias.copy_(b0)
    opt = torch.optim.Adam(fc.parameters(), lr=0.01, weight_decay=1e-4)
    loss_fn = torch.nn.CrossEntropyLoss()
    tr, va, te = (x[split[k]] for k in ("train", "valid", "test"))
    ytr, yva, yte = (y[split[k]] for k in ("train", "valid", "test"))
    best_val, eval_acc = 0, 0
    for _ in range(epochs):
        opt.zero_grad()
        loss_fn(fc(tr), ytr).backward()
        opt.step()
        with torch.no_grad():
            val_acc = (fc(va).argmax(1) == yva).sum().float() / yva.shape[0]
            test_acc = (fc(te).argmax(1) == yte).sum().float() / yte.shape[0]
            if val_acc >= best_val:
                best_val = val_acc
                if test_acc > eval_acc:
                    eval_acc = test_acc
    return float(eval_acc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cora,cs,arxiv,graph")
    ap.add_argument("--runs", default="1,10")
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--interval", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name, acc_fn, f1_fn = host_scores()
    for shape in args.shapes.split(","):
        n, f, c = SHAPES[shape]
        x, y = blobs(n, f, c, 1)
        for r in (int(v) for v in args.runs.split(",")):
            splits = adapters.get_split(n, runs=r, generator=torch.Generator().manual_seed(2))
            dsplits = [{k: v.cuda() for k, v in s.items()} for s in splits]
            w0, b0 = ops.probe_init(r, c, f, torch.Generator().manual_seed(3))
            w0d, b0d = w0.cuda(), b0.cuda()
            sets = [[s[k] for s in dsplits] for k in ("train", "valid", "test")]
            rec = {"shape": shape, "rows": n, "F": f, "C": c, "runs": r, "epochs": args.epochs, "host_scores": name}
            for select, wd in (("scripts", 0.0), ("cca", 1e-4)):
                call = lambda: ops.linear_probe(x, y, *sets, num_classes=c, epochs=args.epochs, weight_decay=wd, test_interval=args.interval,
                                                select=select, weight=w0d, bias=b0d)
                ms, all_ms, res = timed(call, args.reps)
                again = call()
                equal = all(torch.equal(res[k], again[k]) for k in res)
                rec[f"call_{select}_ms"], rec[f"call_{select}_all"], rec[f"call_{select}_equal_bits"] = round(ms, 2), all_ms, equal
                rec[f"call_{select}_stats"] = dict(ops.last_stats)
                rec[f"call_{select}_accuracy"] = [round(v, 4) for v in res["accuracy"].tolist()]
            if not args.no_torch:
                base = lambda: [torch_lr_evaluator(x, y, s, w0d[k], b0d[k], args.epochs, args.interval, acc_fn, f1_fn) for k, s in enumerate(dsplits)]
                ms, all_ms, out = timed(base, args.reps)
                rec["torch_scripts_ms"], rec["torch_scripts_all"] = round(ms, 2), all_ms
                rec["torch_scripts_accuracy"] = [round(float(o["accuracy"]), 4) for o in out]
                base = lambda: [torch_cca_loop(x, y, s, w0d[k], b0d[k], args.epochs) for k, s in enumerate(dsplits)]
                ms, all_ms, out = timed(base, args.reps)
                rec["torch_cca_ms"], rec["torch_cca_all"], rec["torch_cca_accuracy"] = round(ms, 2), all_ms, [round(o, 4) for o in out]
            line = json.dumps(rec)
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
