"""ops.info_nce against a torch restatement of the reference's InfoNCEBatched(tau, batch_size=1024) on the same tensors and the same
device: blocks of 1,024 anchor rows of the N x N cosine-similarity matrix, kept with their exponentials by autograd
for the backward pass.  Forward, and forward + backward (both inputs require gradients).  float32 features, tau = 0.4, the raw
positive term of the script.  Medians of 5 after a warm-up, host clock around a synchronise; the five times are printed too.

Per shape: the times, torch.cuda.max_memory_allocated of either side (reset before it runs; the inputs are part of both figures), and
the fused call's share of the 157 TF peak of the f32 matrix-core instruction, counting 2 N^2 F flops for each of its products: 1
forward, 4 backward (the backward call recomputes the similarities in both of its kernels).

The torch side is run only where an estimate of its working set fits.  A forward pass that records nothing holds three blocks of
1,024 x N float32 (the similarities, their quotient by tau, the exponentials).  Forward + backward: of this restatement autograd keeps
ONE N x N float32 matrix, the result of exp, block by block (the division by a scalar saves nothing, the product saves its (N, F)
inputs, diagonal / sum / log save O(N)); beside it the blocks in flight of both passes, counted as two forward working sets:
4 N^2 + 2 x 3 x 4 x 1,024 x N bytes.  Both estimates are printed beside what torch.cuda.max_memory_allocated then measures.  The
tool works them out first and skips the torch side where one exceeds half of the free memory of the device, so it never runs into
an out-of-memory error on a shared card.  Prints one JSON line per shape (and appends it to --out).  Needs an MI355X; reads
nothing outside the repository.

  cora    : (2708, 256)
  physics : (34493, 256)    Coauthor-Physics
  arxiv   : (169343, 256)   ogbn-arxiv
    python tools/infonce_latency.py
    python tools/infonce_latency.py --shapes physics --no-torch     # the calls alone (for rocprofv3 --kernel-trace --stats)
    python tools/infonce_latency.py --pair                           # one ops.info_nce_pair call against the two calls
    python tools/infonce_latency.py --intraview                      # the plain and the intraview calls, one-way and pair
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
SHAPES = {"cora": (2708, 256), "physics": (34493, 256), "arxiv": (169343, 256)}
TAU = 0.4
BATCH = 1024


def torch_batched(anchor, sample, tau=TAU, batch_size=BATCH):
    """InfoNCEBatched.compute with the identity as the positive mask: the positive term is the similarity, not divided by tau."""
    b = torch.nn.functional.normalize(sample)
    losses = []
    for s in range(0, anchor.shape[0], batch_size):
        sim = torch.nn.functional.normalize(anchor[s:s + batch_size]) @ b.t()
        pos = sim.diagonal(offset=s)
        losses.append(pos - torch.log(torch.exp(sim / tau).sum(dim=1)))
    return -torch.cat(losses).mean()


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
    return statistics.median(ts), [round(t, 3) for t in ts], res


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
    a = torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen)
    b = 0.3 * a + torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen)
    flops = 2.0 * n * n * f
    rec = {"shape": name, "N": n, "F": f, "tau": TAU, "flops_per_product": flops}
    fused = lambda x, y: ops.info_nce(x, y, tau=TAU, positive="raw")
    t, ts, loss, mem = peak_of(lambda: fused(a, b), args.reps)
    st = dict(ops.last_stats)
    rec.update({"forward_ms": round(t, 3), "forward_runs_ms": ts, "forward_of_157TF": round(flops / (t * 1e-3) / PEAK, 4),
                "forward_max_memory_allocated": mem, "forward_arena_bytes": st["arena_bytes"], "parts": st["parts"],
                "host_syncs": st["host_syncs"], "loss": float(loss)})
    rec["repeats_bit_for_bit"] = bool(torch.equal(loss, fused(a, b)))
    t2, ts2, grads, mem2 = peak_of(both_ways(fused, a, b), args.reps)
    rec.update({"forward_backward_ms": round(t2, 3), "forward_backward_runs_ms": ts2,
                "forward_backward_of_157TF": round(5.0 * flops / (t2 * 1e-3) / PEAK, 4), "forward_backward_max_memory_allocated": mem2,
                "backward_arena_bytes": ops.last_stats["arena_bytes"]})
    again = both_ways(fused, a, b)()
    rec["gradients_repeat_bit_for_bit"] = bool(torch.equal(grads[0], again[0]) and torch.equal(grads[1], again[1]))
    del again
    if not args.no_torch:
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        matrix = 4 * n * n
        block = 3 * 4 * min(BATCH, n) * n
        kept = matrix + 2 * block
        rec["torch_bytes_forward_estimate"], rec["torch_bytes_forward_backward_estimate"], rec["free_bytes"] = block, kept, int(free)
        if block <= free // 2:
            tt, tts, want, tmem = peak_of(lambda: torch_batched(a, b), args.reps)
            rec.update({"torch_forward_ms": round(tt, 3), "torch_forward_runs_ms": tts, "torch_forward_over_call": round(tt / t, 3),
                        "torch_forward_max_memory_allocated": tmem, "loss_diff_to_torch": abs(float(loss) - float(want)),
                        "torch_repeats_bit_for_bit": bool(torch.equal(want, torch_batched(a, b)))})
        else:
            rec["torch_forward_ms"] = "not measured: its estimated working set exceeds half of the free memory"
        if kept <= free // 2:
            tt2, tts2, tg, tmem2 = peak_of(both_ways(torch_batched, a, b), args.reps)
            scale = float(max(tg[0].abs().max(), tg[1].abs().max()))
            rec.update({"torch_forward_backward_ms": round(tt2, 3), "torch_forward_backward_runs_ms": tts2,
                        "torch_forward_backward_over_call": round(tt2 / t2, 3), "torch_forward_backward_max_memory_allocated": tmem2,
                        "gradient_diff_to_torch_over_largest": float(max((grads[0] - tg[0]).abs().max(), (grads[1] - tg[1]).abs().max())) / scale})
            del tg
        else:
            rec["torch_forward_backward_ms"] = "not measured: its estimated working set exceeds half of the free memory"
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del a, b, grads
    torch.cuda.empty_cache()


def run_pair(name, n, f, args, fh):
    """--pair: the symmetric loss 0.5 * (l(a, b) + l(b, a)) three ways on the same tensors -- one ops.info_nce_pair call (DESIGN
    4.19), the two ops.info_nce calls of the default NodeContrast, torch's two directions -- forward and forward + backward, with
    the peak memory of each and the largest difference between the pair's result and the two calls'."""
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen)
    b = 0.3 * a + torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen)
    flops = 2.0 * n * n * f
    rec = {"mode": "pair", "shape": name, "N": n, "F": f, "tau": TAU, "flops_per_product": flops}
    pair = lambda x, y: ops.info_nce_pair(x, y, tau=TAU, positive="raw")
    two = lambda x, y: 0.5 * (ops.info_nce(x, y, tau=TAU, positive="raw") + ops.info_nce(y, x, tau=TAU, positive="raw"))
    both = lambda x, y: 0.5 * (torch_batched(x, y) + torch_batched(y, x))
    tp, tsp, lp, memp = peak_of(lambda: pair(a, b), args.reps)
    st = dict(ops.last_stats)
    tw, tsw, lw, memw = peak_of(lambda: two(a, b), args.reps)
    rec.update({"pair_forward_ms": round(tp, 3), "pair_forward_runs_ms": tsp, "pair_forward_of_157TF": round(flops / (tp * 1e-3) / PEAK, 4),
                "pair_forward_max_memory_allocated": memp, "pair_forward_arena_bytes": st["arena_bytes"], "parts": st["parts"],
                "groups": st["groups"], "host_syncs": st["host_syncs"],
                "two_calls_forward_ms": round(tw, 3), "two_calls_forward_runs_ms": tsw, "two_calls_forward_max_memory_allocated": memw,
                "two_calls_forward_over_pair": round(tw / tp, 3), "loss": float(lp), "loss_diff_pair_to_two_calls": abs(float(lp) - float(lw))})
    tp2, tsp2, gp, memp2 = peak_of(both_ways(pair, a, b), args.reps)
    rec["pair_backward_arena_bytes"] = ops.last_stats["arena_bytes"]
    tw2, tsw2, gw, memw2 = peak_of(both_ways(two, a, b), args.reps)
    scale = float(max(gw[0].abs().max(), gw[1].abs().max()))
    rec.update({"pair_forward_backward_ms": round(tp2, 3), "pair_forward_backward_runs_ms": tsp2,
                "pair_forward_backward_of_157TF": round(5.0 * flops / (tp2 * 1e-3) / PEAK, 4), "pair_forward_backward_max_memory_allocated": memp2,
                "two_calls_forward_backward_ms": round(tw2, 3), "two_calls_forward_backward_runs_ms": tsw2,
                "two_calls_forward_backward_max_memory_allocated": memw2, "two_calls_forward_backward_over_pair": round(tw2 / tp2, 3),
                "gradient_diff_pair_to_two_calls_over_largest": float(max((gp[0] - gw[0]).abs().max(), (gp[1] - gw[1]).abs().max())) / scale})
    del gw
    if not args.no_torch:
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        block = 3 * 4 * min(BATCH, n) * n
        kept = 2 * (4 * n * n) + 2 * block                           # autograd keeps the exponentials of both directions
        rec["torch_bytes_forward_estimate"], rec["torch_bytes_forward_backward_estimate"], rec["free_bytes"] = block, kept, int(free)
        if block <= free // 2:
            tt, tts, want, tmem = peak_of(lambda: both(a, b), args.reps)
            rec.update({"torch_forward_ms": round(tt, 3), "torch_forward_runs_ms": tts, "torch_forward_over_pair": round(tt / tp, 3),
                        "torch_forward_max_memory_allocated": tmem, "loss_diff_to_torch": abs(float(lp) - float(want))})
        else:
            rec["torch_forward_ms"] = "not measured: its estimated working set exceeds half of the free memory"
        if kept <= free // 2:
            tt2, tts2, tg, tmem2 = peak_of(both_ways(both, a, b), args.reps)
            tscale = float(max(tg[0].abs().max(), tg[1].abs().max()))
            rec.update({"torch_forward_backward_ms": round(tt2, 3), "torch_forward_backward_runs_ms": tts2,
                        "torch_forward_backward_over_pair": round(tt2 / tp2, 3), "torch_forward_backward_max_memory_allocated": tmem2,
                        "gradient_diff_to_torch_over_largest": float(max((gp[0] - tg[0]).abs().max(), (gp[1] - tg[1]).abs().max())) / tscale})
            del tg
        else:
            rec["torch_forward_backward_ms"] = "not measured: its estimated working set exceeds half of the free memory"
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del a, b, gp
    torch.cuda.empty_cache()


def torch_batched_intra(anchor, sample, variant, tau=TAU, batch_size=BATCH):
    """torch_batched under the sampler with intraview_negs=True: the sample is the (2N, F) concatenation of the sample and the
    anchor; "all" sums every column, as InfoNCEBatched does (it never reads the masks), "masked" takes the anchor's own column out."""
    both = torch.nn.functional.normalize(torch.cat([sample, anchor], dim=0))
    n = anchor.shape[0]
    losses = []
    for s in range(0, n, batch_size):
        sim = torch.nn.functional.normalize(anchor[s:s + batch_size]) @ both.t()
        e = torch.exp(sim / tau)
        total = e.sum(dim=1)
        if variant == "masked":
            total = total - e.diagonal(offset=n + s)
        losses.append(sim.diagonal(offset=s) - torch.log(total))
    return -torch.cat(losses).mean()


def run_intraview(name, n, f, args, fh):
    """--intraview: in one run the plain call and the intraview call, one-way and pair, forward and forward + backward,
    with the peak memory of each, the ratios intraview / plain (8/5 one-way and 11/5 pair by product count, forward + backward) and,
    where its working set fits, torch with the concatenated sample."""
    variant = args.intraview
    gen = torch.Generator(device="cuda").manual_seed(n)
    a = torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen)
    b = 0.3 * a + torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen)
    rec = {"mode": "intraview", "variant": variant, "shape": name, "N": n, "F": f, "tau": TAU, "flops_per_product": 2.0 * n * n * f}
    calls = {
        "plain": lambda x, y: ops.info_nce(x, y, tau=TAU, positive="raw"),
        "intra": lambda x, y: ops.info_nce(x, y, tau=TAU, positive="raw", intraview=variant),
        "pair_plain": lambda x, y: ops.info_nce_pair(x, y, tau=TAU, positive="raw"),
        "pair_intra": lambda x, y: ops.info_nce_pair(x, y, tau=TAU, positive="raw", intraview=variant),
    }
    grads = {}
    for key, fn in calls.items():
        t, ts, loss, mem = peak_of(lambda: fn(a, b), args.reps)
        st = dict(ops.last_stats)
        rec.update({f"{key}_forward_ms": round(t, 3), f"{key}_forward_runs_ms": ts, f"{key}_forward_max_memory_allocated": mem,
                    f"{key}_forward_arena_bytes": st["arena_bytes"], f"{key}_loss": float(loss), f"{key}_host_syncs": st["host_syncs"]})
        t2, ts2, g, mem2 = peak_of(both_ways(fn, a, b), args.reps)
        rec.update({f"{key}_forward_backward_ms": round(t2, 3), f"{key}_forward_backward_runs_ms": ts2,
                    f"{key}_forward_backward_max_memory_allocated": mem2, f"{key}_backward_arena_bytes": ops.last_stats["arena_bytes"]})
        again = both_ways(fn, a, b)()
        rec[f"{key}_gradients_repeat_bit_for_bit"] = bool(torch.equal(g[0], again[0]) and torch.equal(g[1], again[1]))
        if key in ("intra", "pair_intra"):
            grads[key] = g
        del again, g
    for one, base in (("intra", "plain"), ("pair_intra", "pair_plain")):
        rec[f"{one}_over_{base}_forward"] = round(rec[f"{one}_forward_ms"] / rec[f"{base}_forward_ms"], 3)
        rec[f"{one}_over_{base}_forward_backward"] = round(rec[f"{one}_forward_backward_ms"] / rec[f"{base}_forward_backward_ms"], 3)
    if not args.no_torch:
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        block = 3 * 4 * min(BATCH, n) * 2 * n                        # the blocks are 1,024 x 2N
        kept = 4 * n * 2 * n + 2 * block                             # autograd keeps the N x 2N exponentials of a direction
        one_way = lambda x, y: torch_batched_intra(x, y, variant)
        both = lambda x, y: 0.5 * (torch_batched_intra(x, y, variant) + torch_batched_intra(y, x, variant))
        rec["torch_bytes_forward_estimate"], rec["torch_bytes_forward_backward_estimate"], rec["free_bytes"] = block, kept, int(free)
        rec["torch_pair_bytes_forward_backward_estimate"] = 2 * kept
        for key, fn, need, ours in (("torch", one_way, kept, "intra"), ("torch_pair", both, 2 * kept, "pair_intra")):
            if need > free // 2:
                rec[f"{key}_forward_backward_ms"] = "not measured: its estimated working set exceeds half of the free memory"
                continue
            tt, tts, want, tmem = peak_of(lambda: fn(a, b), args.reps)
            rec.update({f"{key}_forward_ms": round(tt, 3), f"{key}_forward_runs_ms": tts, f"{key}_forward_max_memory_allocated": tmem,
                        f"{key}_loss_diff": abs(rec[f"{ours}_loss"] - float(want))})
            tt2, tts2, tg, tmem2 = peak_of(both_ways(fn, a, b), args.reps)
            scale = float(max(tg[0].abs().max(), tg[1].abs().max()))
            g = grads[ours]
            rec.update({f"{key}_forward_backward_ms": round(tt2, 3), f"{key}_forward_backward_runs_ms": tts2,
                        f"{key}_forward_backward_max_memory_allocated": tmem2,
                        f"{key}_forward_backward_over_call": round(tt2 / rec[f"{ours}_forward_backward_ms"], 3),
                        f"{key}_gradient_diff_over_largest": float(max((g[0] - tg[0]).abs().max(), (g[1] - tg[1]).abs().max())) / scale})
            del tg
            torch.cuda.empty_cache()
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del a, b, grads
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pair", action="store_true", help="the symmetric loss: ops.info_nce_pair against the two ops.info_nce calls and torch's two directions")
    ap.add_argument("--intraview", nargs="?", const="masked", default=None, choices=["masked", "all"],
                    help="the plain and the intraview calls, one-way and pair, in one run (the variant: masked by default)")
    ap.add_argument("--shapes", default="cora,physics,arxiv")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    fh = open(args.out, "a") if args.out else None
    for name in args.shapes.split(","):
        n, f = SHAPES[name]
        (run_intraview if args.intraview else run_pair if args.pair else run)(name, n, f, args, fh)


if __name__ == "__main__":
    main()
