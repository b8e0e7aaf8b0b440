"""ops.linear_act against torch on the same tensors and the same device: act(torch.addmm(b, x2d, W)) (x2d @ W for
"none" without a bias) -- the matmul of rocBLAS in whatever summation order it picks, then the activation as an elementwise launch
of its own, and autograd's backward pass, which materialises gy * act'.  Forward, and forward + backward (x, W and b require
gradients).  float32.  Medians of 5 after a warm-up, host clock around a synchronise, the two sides alternating rep by rep; the five
times are printed too.

Per shape: the times, torch.cuda.max_memory_allocated of either side (reset before it runs; the inputs are part of both figures),
whether either side repeats bit for bit over the runs, and for the forward call its algorithmic bytes per second (x read once, y
written once, W and b once) against 8 TB/s and its flops (2 M Fin Fout) against the 157 TF of the f32 matrix-core instruction.
Prints one JSON line per shape (and appends it to --out).  Needs an MI355X; reads nothing outside the repository.

  gin64   : (3, 4,194,304, 64 -> 64) relu, a config-5 GIN layer       gin256 : the same at 256 -> 256
  arxiv   : (2, 169,343, 256 -> 256) elu, the projection head at ogbn-arxiv's size
  cora    : (2, 2,708, 256 -> 256) elu                                 small  : (2, 4,245, 32 -> 32) relu
    python tools/linear_latency.py --out profiles/linear_latency.jsonl
    python tools/linear_latency.py --shapes arxiv --no-torch     # the calls alone (for rocprofv3 --kernel-trace --stats)
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

from rlap_amd import ops  # noqa: E402

PEAK_FLOPS = 157.0e12   # flops per second, v_mfma_f32_32x32x2_f32 on every CU
PEAK_BYTES = 8.0e12     # bytes per second of HBM
SHAPES = {
    "gin64": (3, 4194304, 64, 64, "relu"), "gin256": (3, 4194304, 256, 256, "relu"), "arxiv": (2, 169343, 256, 256, "elu"),
    "cora": (2, 2708, 256, 256, "elu"), "small": (2, 4245, 32, 32, "relu"),
}
ACT = {"none": lambda v: v, "relu": torch.relu, "elu": torch.nn.functional.elu}


def torch_linear(x, w, b, act):
    x2d = x.reshape(-1, x.shape[-1])
    v = torch.addmm(b, x2d, w) if b is not None else x2d @ w
    return ACT[act](v).reshape(x.shape[:-1] + (w.shape[1],))


def forward_of(fn, x, w, b, act):
    return lambda: fn(x, w, b, act)


def both_ways(fn, x, w, b, act, gy):
    def run():
        tx, tw, tb = (t.detach().requires_grad_(True) for t in (x, w, b))
        fn(tx, tw, tb, act).backward(gy)
        return tx.grad, tw.grad, tb.grad
    return run


def equal(res, first):
    pairs = zip(res, first) if isinstance(res, tuple) else [(res, first)]
    return all(bool(torch.equal(p, q)) for p, q in pairs)


def alternating(fns, reps):
    """Each of `fns` once as a warm-up, then `reps` rounds in which they run one after the other: per function (median ms, the
    times, the last result, whether every run gave the warm-up's bits, the peak of allocated memory over its own runs)."""
    first, peaks = [], []
    for fn in fns:                    # the peak of a side alone: nothing of the other side's is alive
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        res = fn()
        torch.cuda.synchronize()
        peaks.append(int(torch.cuda.max_memory_allocated()))
        del res
    for fn in fns:
        first.append(fn())
    torch.cuda.synchronize()
    ts, same, last = [[] for _ in fns], [True] * len(fns), list(first)
    for _ in range(reps):
        for k, fn in enumerate(fns):
            last[k] = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3)
            same[k] = same[k] and equal(res, first[k])
            last[k] = res
    return [(statistics.median(t), [round(v, 3) for v in t], last[k], same[k], peaks[k]) for k, t in enumerate(ts)]


def run(name, shape, args, fh):
    L, n, fin, fout, act = shape
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(L, n, fin, dtype=torch.float32, device="cuda", generator=gen) + 0.25
    w = torch.randn(fin, fout, dtype=torch.float32, device="cuda", generator=gen) / fin ** 0.5
    b = 0.5 * torch.randn(fout, dtype=torch.float32, device="cuda", generator=gen)
    m = L * n
    flops, nbytes = 2.0 * m * fin * fout, 4.0 * (m * fin + m * fout + fin * fout + fout)
    rec = {"shape": name, "L": L, "N": n, "Fin": fin, "Fout": fout, "act": act}
    fused = lambda tx, tw, tb, a: ops.linear_act(tx, tw, tb, act=a)   # noqa: E731
    sides = [forward_of(fused, x, w, b, act)] + ([] if args.no_torch else [forward_of(torch_linear, x, w, b, act)])
    out = alternating(sides, args.reps)
    t, ts, y, same, mem = out[0]
    st = dict(ops.last_stats)
    rec.update({"forward_ms": round(t, 3), "forward_runs_ms": ts, "forward_of_157TF": round(flops / (t * 1e-3) / PEAK_FLOPS, 4),
                "forward_of_8TBs": round(nbytes / (t * 1e-3) / PEAK_BYTES, 4), "forward_max_memory_allocated": mem,
                "forward_arena_bytes": st["arena_bytes"], "host_syncs": st["host_syncs"], "repeats_bit_for_bit": same})
    if not args.no_torch:
        tt, tts, want, tsame, tmem = out[1]
        rec.update({"torch_forward_ms": round(tt, 3), "torch_forward_runs_ms": tts, "torch_forward_over_call": round(tt / t, 3),
                    "torch_forward_max_memory_allocated": tmem, "torch_repeats_bit_for_bit": tsame,
                    "y_diff_to_torch_over_largest": float((y - want).abs().max()) / float(want.abs().max())})
        del want
    del y, out
    gy = torch.randn(L, n, fout, dtype=torch.float32, device="cuda", generator=gen)
    sides = [both_ways(fused, x, w, b, act, gy)] + ([] if args.no_torch else [both_ways(torch_linear, x, w, b, act, gy)])
    out = alternating(sides, args.reps)
    t2, ts2, grads, same2, mem2 = out[0]
    st = dict(ops.last_stats)
    rec.update({"forward_backward_ms": round(t2, 3), "forward_backward_runs_ms": ts2,
                "forward_backward_of_157TF": round(3 * flops / (t2 * 1e-3) / PEAK_FLOPS, 4), "forward_backward_max_memory_allocated": mem2,
                "backward_arena_bytes": st["arena_bytes"], "parts": st["parts"], "gradients_repeat_bit_for_bit": same2})
    if not args.no_torch:
        tt2, tts2, tg, tsame2, tmem2 = out[1]
        rec.update({"torch_forward_backward_ms": round(tt2, 3), "torch_forward_backward_runs_ms": tts2,
                    "torch_forward_backward_over_call": round(tt2 / t2, 3), "torch_forward_backward_max_memory_allocated": tmem2,
                    "torch_gradients_repeat_bit_for_bit": tsame2,
                    "gradient_diff_to_torch_over_largest": max(float((p - q).abs().max()) / float(q.abs().max()) for p, q in zip(grads, tg))})
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del x, gy, grads, out
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
        run(name, SHAPES[name], args, fh)


if __name__ == "__main__":
    main()
