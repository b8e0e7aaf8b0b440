"""ops.bias_act_dropout and ops.layer_norm against torch on the same tensors and the same device: the fused calls
against F.dropout(F.prelu(x + b, a), p) and F.dropout(F.prelu(F.layer_norm(x, (F,), w, b), a), p), forward and forward + backward
(x and every parameter require gradients; the upstream gradient is a fixed random tensor).  float32, training mode, p = 0.2, one
PReLU slope.  Medians of 5 after a warm-up, host clock around a synchronise; the five times are printed too, and both sides' peak
memory above what the inputs hold.

Per shape and call: the times, the algorithmic bytes a second of the fused side against 8 TB/s -- the epilogue reads x and writes y
forward (8 bytes an element) and reads x and gy and writes gx backward (12 more); the layer norm the same forward, and backward 12
for the row pass and 8 for the column sums of the parameter gradients --, and whether two runs gave equal bits (torch draws a new
mask a run, so its side is not compared).  Prints one JSON line per shape and call (and appends it to --out, by default
profiles/rowops_latency.jsonl).  Needs an MI355X; reads nothing outside the repository.

  c5_64, c5_256 : the config-5 batch, L = 3, N = 4,194,304        loader : a DataLoader(batch_size=128) batch, L = 2, N = 4,245, F = 32
  cora, arxiv   : N = 2,708 and 169,343 at F = 256, L = 2
    python tools/rowops_latency.py
    python tools/rowops_latency.py --shapes loader --no-torch      # the calls alone (for rocprofv3 --kernel-trace --stats)
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
import torch.nn.functional as F  # noqa: E402

from rlap_amd import ops  # noqa: E402

PEAK = 8.0e12   # bytes per second
P = 0.2
SHAPES = {"c5_64": (3, 4194304, 64), "c5_256": (3, 4194304, 256), "arxiv": (2, 169343, 256), "cora": (2, 2708, 256), "loader": (2, 4245, 32)}


def timed(fn, reps, compare=True):
    """(median ms, the times, whether every run gave the warm-up's bits, peak bytes above the start)"""
    first = fn()
    torch.cuda.synchronize()
    ts, same = [], True
    torch.cuda.reset_peak_memory_stats()
    start = torch.cuda.memory_allocated()
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        same = same and (not compare or all(bool(torch.equal(x, y)) for x, y in zip(res, first)))
        del res
    return statistics.median(ts), [round(t, 4) for t in ts], same, torch.cuda.max_memory_allocated() - start


def run(name, L, n, f, call, args, fh):
    gen = torch.Generator(device="cuda").manual_seed(n + f)
    x = torch.randn(L, n, f, dtype=torch.float32, device="cuda", generator=gen) + 0.25
    gy = torch.randn(L, n, f, dtype=torch.float32, device="cuda", generator=gen)
    w = 1.0 + 0.1 * torch.randn(f, device="cuda", generator=gen)
    b = 0.1 * torch.randn(f, device="cuda", generator=gen)
    a = torch.full((1,), 0.25, device="cuda")
    elems = L * n * f
    ln = call == "layer_norm"
    rec = {"shape": name, "L": L, "N": n, "F": f, "call": call, "p": P}

    def params():
        return [t.detach().clone().requires_grad_(True) for t in ((w, b, a) if ln else (b, a))]

    def fused(tx, p):
        if ln:
            return ops.layer_norm(tx, p[0], p[1], post="prelu", slope=p[2], p=P, seed=7)
        return ops.bias_act_dropout(tx, p[0], act="prelu", slope=p[1], p=P, seed=7)

    def theirs(tx, p):
        v = F.layer_norm(tx, (f,), p[0], p[1]) if ln else tx + p[0]
        return F.dropout(F.prelu(v.reshape(-1, f), p[-1]).reshape(v.shape), P)

    def both(side):
        def go():
            p = params()
            tx = x.detach().requires_grad_(True)
            side(tx, p).backward(gy)
            return [tx.grad] + [t.grad for t in p]
        return go

    def forward(side):
        def go():
            with torch.no_grad():
                return [side(x, (w, b, a) if ln else (b, a))]
        return go

    t, ts, same, peak = timed(forward(fused), args.reps)
    st = dict(ops.last_stats)
    rec.update({"forward_ms": round(t, 4), "forward_runs_ms": ts, "forward_of_8TBs": round(8.0 * elems / (t * 1e-3) / PEAK, 4), "vec": st["vec"],
                "instance": st["instance"], "launches": st["launches"], "host_syncs": st["host_syncs"], "forward_peak_bytes": peak,
                "repeats_bit_for_bit": same})
    t2, ts2, same2, peak2 = timed(both(fused), args.reps)
    rec.update({"forward_backward_ms": round(t2, 4), "forward_backward_runs_ms": ts2,
                "forward_backward_of_8TBs": round((28.0 if ln else 20.0) * elems / (t2 * 1e-3) / PEAK, 4), "backward_launches": ops.last_stats["launches"],
                "backward_arena_bytes": ops.last_stats["arena_bytes"], "forward_backward_peak_bytes": peak2, "gradients_repeat_bit_for_bit": same2})
    if not args.no_torch:
        torch.cuda.empty_cache()
        tt, tts, _, tpeak = timed(forward(theirs), args.reps, compare=False)
        rec.update({"torch_forward_ms": round(tt, 4), "torch_forward_runs_ms": tts, "torch_forward_over_call": round(tt / t, 3), "torch_forward_peak_bytes": tpeak})
        torch.cuda.empty_cache()
        tt2, tts2, _, tpeak2 = timed(both(theirs), args.reps, compare=False)
        rec.update({"torch_forward_backward_ms": round(tt2, 4), "torch_forward_backward_runs_ms": tts2,
                    "torch_forward_backward_over_call": round(tt2 / t2, 3), "torch_forward_backward_peak_bytes": tpeak2})
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del x, gy
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rowops_latency.jsonl"), help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    fh = open(args.out, "a") if args.out else None
    for name in args.shapes.split(","):
        L, n, f = SHAPES[name]
        for call in ("bias_act_dropout", "layer_norm"):
            run(name, L, n, f, call, args, fh)


if __name__ == "__main__":
    main()
