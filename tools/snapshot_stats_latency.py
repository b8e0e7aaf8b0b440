"""Time ops.snapshot_stats next to the depths call that produced its snapshots.

  ba1m : BA(1M, 10), depths [N/8, N/4, N/2], views=2 (6 snapshots, all in the large regime)
  c5   : bench config 5, a node_ptr batch of 1024 x BA(4096, 8), depths [n/8, n/4, n/2] (3,072 snapshots, all small)
Prints one JSON line per graph: median ms of the depths call and of the stats call (host clock around a synchronise), the stats
call's rlap_snapshot_info (Lanczos steps, host synchronisations), and how many snapshots converged.  Run it under
`rocprofv3 --kernel-trace --stats` for kernel times.
  python tools/snapshot_stats_latency.py --graphs ba1m,c5 --reps 5
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GRAPHS = {"ba1m": (1000000, 10, 1, 2), "c5": (4096, 8, 1024, 1)}   # (nodes per graph, m, graphs, views)


def run(name, reps):
    import torch
    from rlap_amd import graphs, ops
    n, m, G, K = GRAPHS[name]
    e1 = graphs.barabasi_albert(n, m, 1)
    ei = (torch.cat([e1 + g * n for g in range(G)], dim=1) if G > 1 else e1).cuda()
    N = G * n
    node_ptr = [g * n for g in range(G + 1)] if G > 1 else None
    ts = [n // 8, n // 4, n // 2]

    def depths():
        return ops.approximate_cholesky_depths(ei, None, N, ts, "random", "asc", node_ptr=node_ptr, views=K, seed=1234)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return r, (time.perf_counter() - t0) * 1e3
    (sc, ptr), _ = timed(depths)   # (warm-up)
    st, _ = timed(lambda: ops.snapshot_stats(sc, ptr, N, node_ptr=node_ptr))
    td, ts_ = [], []
    for _ in range(reps):
        (sc, ptr), t = timed(depths)
        td.append(t)
        st, t = timed(lambda: ops.snapshot_stats(sc, ptr, N, node_ptr=node_ptr))
        ts_.append(t)
        info = dict(ops.last_stats)
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps({"graph": name, "snapshots": int(ptr.numel() - 1), "rows": int(ptr[-1]), "depths_ms": round(med(td), 2),
                      "stats_ms": round(med(ts_), 2), "info": info, "converged": int(st["converged"].sum()),
                      "iters_max": int(st["iters"].max()), "iters_mean": round(float(st["iters"].float().mean()), 1),
                      "lambda_max": [round(float(x), 6) for x in st["lambda_max"][:6].cpu()]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ba1m,c5")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    for g in a.graphs.split(","):
        run(g, a.reps)


if __name__ == "__main__":
    main()
