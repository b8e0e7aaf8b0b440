"""ops.g2l_jsd and ops.g2l_bootstrap against a torch restatement of the reference's lines on the same tensors and the same device
(DESIGN 4.17): JSD.compute of scripts/node_dedicated.py with the graph-to-local sampler's dense (G, N) masks (one graph: the
concatenated [h; neg] copy), and BootstrapLatent with the dense (G, N) positive mask.  Forward, and forward + backward (every input
that has a gradient requires it).  float32 features.  Medians of 5 after a warm-up, host clock around a synchronise; the five times
are printed too.

Per shape: the times, torch.cuda.max_memory_allocated of either side (reset before it runs; the inputs are part of both figures),
the losses of both sides, whether the fused side repeats bit for bit over the runs.  Prints one JSON line per shape (and appends it
to --out).  Needs an MI355X; reads nothing outside the repository.

  one graph with neg : cora 2,708 nodes, physics 34,493 (Coauthor-Physics), arxiv 169,343 (ogbn-arxiv); F = 256 and 512
  batch128           : 4,245 nodes in 128 graphs, F = 32 (a DataLoader(batch_size=128)-like batch); JSD and bootstrap
  config5            : 4,194,304 nodes in 1,024 graphs, F = 64; JSD and bootstrap
    python tools/g2l_latency.py
    python tools/g2l_latency.py --shapes batch128 --no-torch     # the calls alone (for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from rlap_amd import ops  # noqa: E402

NODES = {"cora": 2708, "physics": 34493, "arxiv": 169343}
# name -> (N, G, F, losses)
SHAPES = {f"{name}{f}": (n, 1, f, ("jsd",)) for f in (256, 512) for name, n in NODES.items()}
SHAPES["batch128"] = (4245, 128, 32, ("jsd", "bootstrap"))
SHAPES["config5"] = (4194304, 1024, 64, ("jsd", "bootstrap"))


def torch_jsd(h, g, batch, neg):
    """JSD.compute on the sampler's masks: anchor = the summaries, sample = the nodes (one graph: [h; neg])."""
    n = h.shape[0]
    if neg is not None:
        sample = torch.cat([h, neg], dim=0)
        pos = torch.cat([torch.ones(1, n, device=h.device), torch.zeros(1, n, device=h.device)], dim=1)
    else:
        sample = h
        pos = torch.zeros(g.shape[0], n, device=h.device)
        pos[batch, torch.arange(n, device=h.device)] = 1.0
    neg_mask = 1.0 - pos
    num_neg, num_pos = neg_mask.int().sum(), pos.int().sum()
    similarity = g @ sample.t()
    e_pos = (math.log(2) - torch.nn.functional.softplus(-similarity * pos)).sum() / num_pos
    neg_sim = similarity * neg_mask
    e_neg = (torch.nn.functional.softplus(-neg_sim) + neg_sim - math.log(2)).sum() / num_neg
    return e_neg - e_pos


def torch_bootstrap(h, g, batch, _neg):
    n = h.shape[0]
    pos = torch.zeros(g.shape[0], n, device=h.device)
    pos[batch, torch.arange(n, device=h.device)] = 1.0
    similarity = torch.nn.functional.normalize(g, dim=-1, p=2) @ torch.nn.functional.normalize(h, dim=-1, p=2).t()
    return (similarity * pos).sum(dim=-1).mean()


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


def peak_of(fn, reps):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    out = timed(fn, reps)
    return out + (int(torch.cuda.max_memory_allocated()),)


def both_ways(loss_fn, tensors):
    """forward + backward: every tensor of `tensors` that is not None requires a gradient; returns the gradients"""
    def run():
        leaves = [t.detach().requires_grad_(True) if t is not None else None for t in tensors]
        loss_fn(*leaves).backward()
        return tuple(t.grad for t in leaves if t is not None)
    return run


def run(name, n, G, f, loss, args, fh):
    gen = torch.Generator(device="cuda").manual_seed(n)
    h = 0.5 * torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen)
    g = torch.randn(G, f, dtype=torch.float32, device="cuda", generator=gen)
    neg = 0.5 * torch.randn(n, f, dtype=torch.float32, device="cuda", generator=gen) if (G == 1 and loss == "jsd") else None
    table = ops.GraphTable([(n * j) // G for j in range(G + 1)], n)
    batch = torch.repeat_interleave(torch.arange(G, device="cuda"), (table.host[1:] - table.host[:-1]).cuda())
    rec = {"shape": name, "loss_kind": loss, "N": n, "G": G, "F": f}
    if loss == "jsd":
        fused = lambda x, y, z: ops.g2l_jsd(x, y, node_ptr=table, neg=z)
        ref = lambda x, y, z: torch_jsd(x, y, batch, z)
        leaves = (h, g, neg)
    else:
        fused = lambda x, y, z: ops.g2l_bootstrap(x, y.detach() if y.requires_grad else y, node_ptr=table)
        ref = lambda x, y, z: torch_bootstrap(x, y.detach(), batch, z)
        leaves = (h, None, None)
    call = lambda fn: (lambda: fn(h, g, neg))
    back = lambda fn: both_ways((lambda x, y, z: fn(x, y if y is not None else g, z)), leaves)
    t, ts, value, same, mem = peak_of(call(fused), args.reps)
    st = dict(ops.last_stats)
    rec.update({"forward_ms": round(t, 3), "forward_runs_ms": ts, "forward_max_memory_allocated": mem, "forward_arena_bytes": st["arena_bytes"],
                "parts": st["parts"], "host_syncs": st["host_syncs"], "loss": float(value), "repeats_bit_for_bit": same})
    t2, ts2, grads, same2, mem2 = peak_of(back(fused), args.reps)
    rec.update({"forward_backward_ms": round(t2, 3), "forward_backward_runs_ms": ts2, "forward_backward_max_memory_allocated": mem2,
                "backward_arena_bytes": ops.last_stats["arena_bytes"], "gradients_repeat_bit_for_bit": same2})
    if not args.no_torch:
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info()
        kept = 12 * 4 * max(G, 2) * n + 8 * 4 * n * f       # the masks, the similarities, their products and gradients, generously
        rec["free_bytes"] = int(free)
        if kept <= free // 2:
            tt, tts, want, tsame, tmem = peak_of(call(ref), args.reps)
            rec.update({"torch_forward_ms": round(tt, 3), "torch_forward_runs_ms": tts, "torch_forward_over_call": round(tt / t, 3),
                        "torch_forward_max_memory_allocated": tmem, "torch_loss": float(want),
                        "loss_diff_to_torch": abs(float(value) - float(want)), "torch_repeats_bit_for_bit": tsame})
            tt2, tts2, tg, tsame2, tmem2 = peak_of(back(ref), args.reps)
            scale = float(max(x.abs().max() for x in tg))
            rec.update({"torch_forward_backward_ms": round(tt2, 3), "torch_forward_backward_runs_ms": tts2,
                        "torch_forward_backward_over_call": round(tt2 / t2, 3), "torch_forward_backward_max_memory_allocated": tmem2,
                        "torch_gradients_repeat_bit_for_bit": tsame2,
                        "gradient_diff_to_torch_over_largest": float(max((x - y).abs().max() for x, y in zip(grads, tg))) / scale})
            del tg
        else:
            rec["torch_forward_ms"] = "not measured: its estimated working set exceeds half of the free memory"
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del h, g, neg, grads
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
        n, G, f, losses = SHAPES[name]
        for loss in losses:
            run(name, n, G, f, loss, args, fh)


if __name__ == "__main__":
    main()
