"""ops.barlow_twins_loss against a torch restatement of the published bt_loss (PyGCL's L.BarlowTwins) on the same tensors and the
same device: the standardisation of both views, one F x F product over all N nodes forward (rocBLAS, in whatever
summation order it picks) and two more in autograd's backward pass.  Forward, and forward + backward (both inputs require
gradients).  float32 features, lambd = 1 / F.  Medians of 5 after a warm-up, host clock around a synchronise; the five times are
printed too.

Per shape: the times, torch.cuda.max_memory_allocated of either side (reset before it runs; the inputs are part of both figures),
whether either side repeats bit for bit over the runs, and the fused call's share of the 157 TF peak of the f32 matrix-core
instruction, counting the multiply-adds it issues as 2 flops: about Fp^2 N forward (one full product; a clamped tile is counted
too) and 2 x Fp^2 N backward.  Prints one JSON line per shape (and appends it to --out).  Needs an MI355X; reads nothing outside
the repository.

  cora    : 2,708 nodes     physics : 34,493 (Coauthor-Physics)     arxiv : 169,343 (ogbn-arxiv);  F = 512 and 256
    python tools/bt_latency.py
    python tools/bt_latency.py --shapes physics512 --no-torch     # the calls alone (for rocprofv3 --kernel-trace --stats)
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

PEAK = 157.0e12   # flops per second, v_mfma_f32_32x32x2_f32 on every CU
NODES = {"cora": 2708, "physics": 34493, "arxiv": 169343}
SHAPES = {f"{name}{f}": (n, f) for f in (512, 256) for name, n in NODES.items()}
EPS = 1e-15


def torch_bt(h1, h2, lambd=None, eps=EPS):
    z1 = (h1 - h1.mean(0)) / (h1.std(0) + eps)
    z2 = (h2 - h2.mean(0)) / (h2.std(0) + eps)
    n, f = h1.shape
    lambd = 1.0 / f if lambd is None else lambd
    c = torch.mm(z1.T, z2) / n
    off = ~torch.eye(f, dtype=torch.bool, device=h1.device)
    return (1 - c.diagonal()).pow(2).sum() + lambd * c[off].pow(2).sum()


def timed(fn, reps):
    """(median ms, the times, the last result, whether every run gave the warm-up's bits)"""
    first = fn()
    torch.cuda.synchronize()
    ts, same = [], True
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
        pairs = zip(res, first) if isinstance(res, tuple) else [(res, first)]
        same = same and all(bool(torch.equal(x, y)) or bool(torch.isnan(x).all() and torch.isnan(y).all()) for x, y in pairs)
    return statistics.median(ts), [round(t, 3) for t in ts], res, same


def both_ways(loss_fn, a, b):
    def run():
        ta, tb = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
        loss_fn(ta, tb).backward()
        return ta.grad, tb.grad
    return run


def peak_of(fn, reps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = timed(fn, reps)
    return out + (int(torch.cuda.max_memory_allocated()),)


def run(name, n, f, args, fh):
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen) + 0.5
    b = 0.6 * a.roll(-1, 1) + 0.4 * torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen) + 1.0
    fp = (f + 31) // 32 * 32
    tiles = (fp // 32 + 1) // 2 * 2                       # the tiles a wave row computes: a clamped one too
    fwd_flops, bwd_flops = 2.0 * n * (32 * tiles) ** 2, 2.0 * 2 * n * fp * fp
    rec = {"shape": name, "N": n, "F": f, "lambd": 1.0 / f, "eps": EPS}
    fused = lambda x, y: ops.barlow_twins_loss(x, y)      # noqa: E731
    t, ts, loss, same, mem = peak_of(lambda: fused(a, b), args.reps)
    st = dict(ops.last_stats)
    rec.update({"forward_ms": round(t, 3), "forward_runs_ms": ts, "forward_of_157TF": round(fwd_flops / (t * 1e-3) / PEAK, 4),
                "forward_max_memory_allocated": mem, "forward_arena_bytes": st["arena_bytes"], "parts": st["parts"],
                "host_syncs": st["host_syncs"], "loss": float(loss), "repeats_bit_for_bit": same})
    t2, ts2, grads, same2, mem2 = peak_of(both_ways(fused, a, b), args.reps)
    rec.update({"forward_backward_ms": round(t2, 3), "forward_backward_runs_ms": ts2,
                "forward_backward_of_157TF": round((fwd_flops + bwd_flops) / (t2 * 1e-3) / PEAK, 4), "forward_backward_max_memory_allocated": mem2,
                "backward_arena_bytes": ops.last_stats["arena_bytes"], "gradients_repeat_bit_for_bit": same2})
    if not args.no_torch:
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        kept = 12 * 4 * n * f            # z, the centred copies and the gradients of both views, generously
        rec["free_bytes"] = int(free)
        if kept <= free // 2:
            tt, tts, want, tsame, tmem = peak_of(lambda: torch_bt(a, b), args.reps)
            rec.update({"torch_forward_ms": round(tt, 3), "torch_forward_runs_ms": tts, "torch_forward_over_call": round(tt / t, 3),
                        "torch_forward_max_memory_allocated": tmem, "loss_diff_to_torch_relative": abs(float(loss) - float(want)) / abs(float(want)),
                        "torch_repeats_bit_for_bit": tsame})
            tt2, tts2, tg, tsame2, tmem2 = peak_of(both_ways(torch_bt, a, b), args.reps)
            scale = float(max(tg[0].abs().max(), tg[1].abs().max()))
            rec.update({"torch_forward_backward_ms": round(tt2, 3), "torch_forward_backward_runs_ms": tts2,
                        "torch_forward_backward_over_call": round(tt2 / t2, 3), "torch_forward_backward_max_memory_allocated": tmem2,
                        "torch_gradients_repeat_bit_for_bit": tsame2,
                        "gradient_diff_to_torch_over_largest": float(max((grads[0] - tg[0]).abs().max(), (grads[1] - tg[1]).abs().max())) / scale})
            del tg
        else:
            rec["torch_forward_ms"] = "not measured: its estimated working set exceeds half of the free memory"
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del a, b, grads
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
        n, f = SHAPES[name]
        run(name, n, f, args, fh)


if __name__ == "__main__":
    main()
