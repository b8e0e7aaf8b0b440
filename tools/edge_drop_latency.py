"""ops.drop_edges against a torch restatement of the reference's lines on the same device and tensors.  The four
schemes with K = 2 views -- one call here, two `augment` calls of the restatement, as the training scripts make them -- on BA(1M, 10)
and on the disjoint union of the batch of bench config 5 (1,024 BA(4096, 8) graphs).  The restatement follows
scripts/augmentor_benchmarks.py:216-363 in float32 with index_add_ for scatter and unique for to_undirected's coalesce; for the
eigenvector scheme it runs the same power iteration in torch (one .item() a step for the stopping test; float32 like the other arms,
with --float64-too in float64 beside it), since networkx is not assumed.  Medians of 5 after a warm-up, host clock around a
synchronise; the five times are printed too.  Prints one JSON line per (graph, scheme) (and appends it to --out).  `flip_bytes` is what the flip-and-compact kernels must move at least: the ids (and
weights) of every row read once, 24 bytes written per kept row; their own times come from a kernel trace of a --no-torch run
(k_rc_count<DropCoin> + k_rc_write<DropCoin>) and are set against 8 TB/s in DESIGN 4.20.  Needs an MI355X; reads nothing outside the repository.

    python tools/edge_drop_latency.py
    python tools/edge_drop_latency.py --graphs ba --schemes uniform,degree --no-torch   # the calls alone (for a kernel trace)
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

from rlap_amd import graphs, ops  # noqa: E402

PEAK = 8.0e12   # bytes per second, the HBM specification
PS, THRESHOLD = (0.3, 0.4), 0.7


def make(name):
    if name == "ba":
        ei = graphs.barabasi_albert(1_000_000, 10, 1)
        return ei.cuda(), 1_000_000
    parts = [graphs.barabasi_albert(4096, 8, 1 + g) + 4096 * g for g in range(1024)]
    return torch.cat(parts, 1).cuda(), 4096 * 1024


def timed(fn, reps=5):
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


# ---- the reference's lines, restated in torch
def t_degree(index, n):
    return torch.zeros(n, dtype=torch.float32, device=index.device).index_add_(0, index, torch.ones(index.numel(), dtype=torch.float32, device=index.device))


def t_drop_weighted(weights, p, threshold):
    weights = weights / weights.mean() * p
    weights = weights.where(weights < threshold, torch.ones_like(weights) * threshold)
    return torch.bernoulli(1.0 - weights).to(torch.bool)


def t_degree_weights(ei, n):
    key = torch.unique(torch.cat([ei[1], ei[0]]) * n + torch.cat([ei[0], ei[1]]))      # to_undirected: both directions, coalesced
    s = torch.log(t_degree(key // n, n)[ei[1]])
    return (s.max() - s) / (s.max() - s.mean())


def t_pr_weights(ei, n, damp=0.85, k=10):
    deg_out = t_degree(ei[0], n)
    x = torch.ones(n, dtype=torch.float32, device=ei.device)
    for _ in range(k):
        msg = x[ei[0]] / deg_out[ei[0]]
        x = (1 - damp) * x + damp * torch.zeros_like(x).index_add_(0, ei[1], msg)
    s = torch.log(x[ei[1]])
    return (s.max() - s) / (s.max() - s.mean())


def t_evc_weights(ei, n, tol=1e-6, max_iter=1000, dtype=torch.float32):
    x = torch.full((n,), n ** -0.5, dtype=dtype, device=ei.device)
    for _ in range(max_iter):
        y = x.clone().index_add_(0, ei[1], x[ei[0]])
        y = y / y.norm()
        err = (y - x).abs().sum().item()
        x = y
        if err <= n * tol:
            break
    x = x.float()
    s = (x.where(x > 0, torch.zeros_like(x)) + 1e-8).log()[ei[1]]
    return (s.max() - s) / (s.max() - s.mean())


def t_augment(ei, n, scheme, p, **kw):
    if scheme == "uniform":
        mask = torch.bernoulli(torch.full((ei.shape[1],), 1.0 - p, device=ei.device)).to(torch.bool)
    else:
        w = {"degree": t_degree_weights, "pagerank": t_pr_weights, "eigenvector": t_evc_weights}[scheme](ei, n, **kw)
        mask = t_drop_weighted(w, p, THRESHOLD)
    return ei[:, mask]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ba,c5")
    ap.add_argument("--schemes", default="uniform,degree,pagerank,eigenvector")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--float64-too", action="store_true", help="eigenvector: torch's power iteration in float64 as well (seconds a run)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    fh = open(args.out, "a") if args.out else None
    for gname in args.graphs.split(","):
        ei, n = make(gname)
        E = int(ei.shape[1])
        for scheme in args.schemes.split(","):
            rec = {"graph": gname, "N": n, "E": E, "scheme": scheme, "K": len(PS), "p": list(PS), "threshold": THRESHOLD}
            t, ts, res = timed(lambda: ops.drop_edges(ei, None, n, list(PS), scheme, THRESHOLD, seed=1), args.reps)
            st = dict(ops.last_stats)
            M = int(res[0].shape[0])
            rec.update({"call_ms": round(t, 3), "call_runs_ms": ts, "kept_rows": M, "iters": st["iters"], "converged": st["converged"],
                        "launches": st["launches"], "host_syncs": st["host_syncs"], "arena_bytes": st["arena_bytes"], "flip_bytes": 16 * E + 24 * M})
            t1, ts1, _ = timed(lambda: ops.drop_edges(ei, None, n, PS[0], scheme, THRESHOLD, seed=1), args.reps)
            rec.update({"one_view_ms": round(t1, 3), "one_view_runs_ms": ts1})
            del res
            if not args.no_torch:
                tt, tst, got = timed(lambda: [t_augment(ei, n, scheme, p) for p in PS], args.reps)
                rec.update({"torch_dtype": "float32", "torch_two_augments_ms": round(tt, 3), "torch_runs_ms": tst, "torch_over_call": round(tt / t, 3),
                            "torch_kept_rows": int(sum(g.shape[1] for g in got))})
                del got
                if scheme == "eigenvector" and args.float64_too:   # the call's own precision beside it: the power iteration in float64
                    t64, ts64, _ = timed(lambda: [t_augment(ei, n, scheme, p, dtype=torch.float64) for p in PS], args.reps)
                    rec.update({"torch_float64_two_augments_ms": round(t64, 3), "torch_float64_runs_ms": ts64, "torch_float64_over_call": round(t64 / t, 3)})
            line = json.dumps(rec)
            print(line, flush=True)
            if fh is not None:
                fh.write(line + "\n")
                fh.flush()
            torch.cuda.empty_cache()
        del ei
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
