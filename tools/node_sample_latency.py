"""ops.sample_subgraphs against a torch restatement of PyGCL's lines on the same device and tensors.  The two schemes
with K = 2 views -- one call here, two `augment` calls of the restatement, as the training scripts make them -- on BA(1M, 10) and on
the disjoint union of the batch of bench config 5 (1,024 BA(4096, 8) graphs).  "drop" at p = (0.3, 0.4); "walk" at
num_seeds = (0.3 N, 0.4 N), walk_length = 10.  The restatement: NodeDropping is a bernoulli over the nodes and subgraph's mask and
gather; RWSampling builds a CSR with sort, takes walk_length steps `col[rowptr[cur] + floor(rand * deg)]` (a walker on a node
without outgoing rows stays), marks the visited nodes and filters as subgraph does -- torch_sparse and torch_cluster are not
assumed.  Medians of 5 after a warm-up, host clock around a synchronise; the five times are printed too.  Prints one JSON line per
(graph, scheme) (and appends it to --out).  `flip_bytes` is what the flip-and-compact kernels must move at least: the two ids of
every row read once, 24 bytes written per kept row; their own times come from a kernel trace of a --no-torch run (k_rc_count +
k_rc_write, of the predicate NodeCoins for drop and InWalk for walk) and are set against 8 TB/s in DESIGN 4.21; `walker_steps` over k_ns_walk's time is the walk kernel's rate.  Needs an
MI355X; reads nothing outside the repository.

    python tools/node_sample_latency.py
    python tools/node_sample_latency.py --graphs ba --schemes drop --no-torch   # the calls alone (for a kernel trace)
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
PS, FRACTIONS, WALK_LENGTH = (0.3, 0.4), (0.3, 0.4), 10


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


# ---- PyGCL's lines, restated in torch
def t_subgraph(ei, keep):
    """torch_geometric.utils.subgraph with a bool subset and relabel_nodes=False."""
    mask = keep[ei[0]] & keep[ei[1]]
    return ei[:, mask]


def t_node_dropping(ei, n, pn):
    keep = torch.bernoulli(torch.full((n,), 1.0 - pn, device=ei.device)).to(torch.bool)
    return t_subgraph(ei, keep)


def t_rw_sampling(ei, n, num_seeds, walk_length):
    order = torch.sort(ei[0], stable=True)[1]
    col = ei[1][order]
    deg = torch.bincount(ei[0], minlength=n)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=ei.device)
    rowptr[1:] = torch.cumsum(deg, 0)
    cur = torch.randint(0, n, (num_seeds,), device=ei.device)
    keep = torch.zeros(n, dtype=torch.bool, device=ei.device)
    keep[cur] = True
    for _ in range(walk_length):
        d = deg[cur]
        nxt = col[(rowptr[cur] + (torch.rand(num_seeds, device=ei.device) * d).long()).clamp_(max=col.numel() - 1)]   # (d = 0 may point past the end)
        cur = torch.where(d > 0, nxt, cur)
        keep[cur] = True
    return t_subgraph(ei, keep)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ba,c5")
    ap.add_argument("--schemes", default="drop,walk")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    fh = open(args.out, "a") if args.out else None
    for gname in args.graphs.split(","):
        ei, n = make(gname)
        E = int(ei.shape[1])
        seeds = [int(f * n) for f in FRACTIONS]
        for scheme in args.schemes.split(","):
            kw = {"p": list(PS)} if scheme == "drop" else {"num_seeds": seeds, "walk_length": WALK_LENGTH}
            one = {"p": PS[0]} if scheme == "drop" else {"num_seeds": seeds[0], "walk_length": WALK_LENGTH}
            rec = {"graph": gname, "N": n, "E": E, "scheme": scheme, "K": 2, **kw}
            t, ts, res = timed(lambda: ops.sample_subgraphs(ei, None, n, scheme, seed=1, **kw), args.reps)
            st = dict(ops.last_stats)
            M = int(res[0].shape[0])
            rec.update({"call_ms": round(t, 3), "call_runs_ms": ts, "kept_rows": M, "launches": st["launches"], "host_syncs": st["host_syncs"],
                        "arena_bytes": st["arena_bytes"], "flip_bytes": 16 * E + 24 * M})
            if scheme == "walk":
                rec["walker_steps"] = sum(seeds) * WALK_LENGTH
            t1, ts1, _ = timed(lambda: ops.sample_subgraphs(ei, None, n, scheme, seed=1, **one), args.reps)
            rec.update({"one_view_ms": round(t1, 3), "one_view_runs_ms": ts1})
            del res
            if not args.no_torch:
                if scheme == "drop":
                    tt, tst, got = timed(lambda: [t_node_dropping(ei, n, p) for p in PS], args.reps)
                else:
                    tt, tst, got = timed(lambda: [t_rw_sampling(ei, n, s, WALK_LENGTH) for s in seeds], args.reps)
                rec.update({"torch_two_augments_ms": round(tt, 3), "torch_runs_ms": tst, "torch_over_call": round(tt / t, 3),
                            "torch_kept_rows": int(sum(g.shape[1] for g in got))})
                del got
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
