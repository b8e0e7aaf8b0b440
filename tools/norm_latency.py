"""ops.batch_norm against torch on the same tensors and the same device: the fused per-view call with pre="relu" (and
post="prelu") for all L layers at once against F.batch_norm(F.relu(x[l]), ...) per layer (and F.prelu behind it), forward and
forward + backward (x, weight, bias and the slope require gradients; the upstream gradient is a fixed random tensor).  float32,
training mode, running buffers updated.  Medians of 5 after a warm-up, host clock around a synchronise; the five times are printed too.

Per shape: the times, the algorithmic bytes a second of either side against 8 TB/s -- the fused call reads x twice and writes y once
forward (12 bytes an element) and reads x and gy twice and writes gx once backward (20 more); torch's relu reads and writes once and
its batch_norm reads twice and writes once (20 bytes an element forward, 28 with the prelu) --, and whether two runs gave equal bits,
on both sides.  Prints one JSON line per shape and activation (and appends it to --out).  Needs an MI355X; reads nothing outside the
repository.

  c5_64, c5_256 : the config-5 batch, L = 3, N = 4,194,304        loader : a DataLoader(batch_size=128) batch, L = 2, N = 4,245, F = 32
  cora, arxiv   : N = 2,708 and 169,343 at F = 256, L = 2
    python tools/norm_latency.py
    python tools/norm_latency.py --shapes loader --no-torch        # the calls alone (for rocprofv3 --kernel-trace --stats)
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
SHAPES = {"c5_64": (3, 4194304, 64), "c5_256": (3, 4194304, 256), "loader": (2, 4245, 32), "cora": (2, 2708, 256), "arxiv": (2, 169343, 256)}


def timed(fn, reps):
    """(median ms, the times, whether every run gave the warm-up's bits)"""
    first = fn()
    torch.cuda.synchronize()
    ts, same = [], True
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        same = same and all(bool(torch.equal(x, y)) for x, y in zip(res, first))
        del res
    return statistics.median(ts), [round(t, 4) for t in ts], same


def run(name, L, n, f, prelu, args, fh):
    gen = torch.Generator(device="cuda").manual_seed(n + f)
    x = torch.randn(L, n, f, dtype=torch.float32, device="cuda", generator=gen) + 0.25
    gy = torch.randn(L, n, f, dtype=torch.float32, device="cuda", generator=gen)
    w = 1.0 + 0.1 * torch.randn(f, device="cuda", generator=gen)
    b = 0.1 * torch.randn(f, device="cuda", generator=gen)
    a = torch.full((1,), 0.25, device="cuda")
    elems = L * n * f
    rec = {"shape": name, "L": L, "N": n, "F": f, "post": "prelu" if prelu else "none"}

    def params():
        return [t.detach().clone().requires_grad_(True) for t in ((w, b, a) if prelu else (w, b))]

    def fused_forward():
        rm, rv = torch.zeros(f, device="cuda"), torch.ones(f, device="cuda")
        return ops.batch_norm(x, w, b, rm, rv, pre="relu", post="prelu" if prelu else "none", slope=a if prelu else None), rm, rv

    def fused_both():
        p = params()
        tx = x.detach().requires_grad_(True)
        ops.batch_norm(tx, p[0], p[1], pre="relu", post="prelu" if prelu else "none", slope=p[2] if prelu else None).backward(gy)
        return [tx.grad] + [t.grad for t in p]

    def torch_layers(tx, p, rm, rv):
        ys = []
        for l in range(L):
            y = F.batch_norm(F.relu(tx[l]), rm, rv, p[0], p[1], True, 0.1, 1e-5)
            ys.append(F.prelu(y, p[2]) if prelu else y)
        return ys

    def torch_forward():
        rm, rv = torch.zeros(f, device="cuda"), torch.ones(f, device="cuda")
        with torch.no_grad():
            return torch_layers(x, (w, b, a), rm, rv) + [rm, rv]

    def torch_both():
        p = params()
        tx = x.detach().requires_grad_(True)
        torch.autograd.backward(torch_layers(tx, p, None, None), [gy[l] for l in range(L)])
        return [tx.grad] + [t.grad for t in p]

    t, ts, same = timed(fused_forward, args.reps)
    st = dict(ops.last_stats)
    rec.update({"forward_ms": round(t, 4), "forward_runs_ms": ts, "forward_of_8TBs": round(12.0 * elems / (t * 1e-3) / PEAK, 4), "vec": st["vec"],
                "launches": st["launches"], "arena_bytes": st["arena_bytes"], "host_syncs": st["host_syncs"], "repeats_bit_for_bit": same})
    t2, ts2, same2 = timed(fused_both, args.reps)
    rec.update({"forward_backward_ms": round(t2, 4), "forward_backward_runs_ms": ts2, "forward_backward_of_8TBs": round(32.0 * elems / (t2 * 1e-3) / PEAK, 4),
                "backward_launches": ops.last_stats["launches"], "gradients_repeat_bit_for_bit": same2})
    if not args.no_torch:
        torch.cuda.empty_cache()
        tt, tts, tsame = timed(torch_forward, args.reps)
        rec.update({"torch_forward_ms": round(tt, 4), "torch_forward_runs_ms": tts, "torch_forward_over_call": round(tt / t, 3),
                    "torch_forward_of_8TBs": round((28.0 if prelu else 20.0) * elems / (tt * 1e-3) / PEAK, 4), "torch_repeats_bit_for_bit": tsame})
        torch.cuda.empty_cache()
        tt2, tts2, tsame2 = timed(torch_both, args.reps)
        rec.update({"torch_forward_backward_ms": round(tt2, 4), "torch_forward_backward_runs_ms": tts2,
                    "torch_forward_backward_over_call": round(tt2 / t2, 3), "torch_gradients_repeat_bit_for_bit": tsame2})
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
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    fh = open(args.out, "a") if args.out else None
    for name in args.shapes.split(","):
        L, n, f = SHAPES[name]
        for prelu in (False, True):
            run(name, L, n, f, prelu, args, fh)


if __name__ == "__main__":
    main()
