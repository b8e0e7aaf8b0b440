"""Latency of nested Schur complements, for the same graph, seed and depths [n/8, n/4, n/2], against the calls they replace:
  separate : D calls without depths, one per depth (ops.approximate_cholesky; with --views K > 1 or a batch,
             ops.approximate_cholesky_views with that depth for every (view, graph))
  deepest  : the one such call at the deepest depth (what the depths call should cost, plus D-1 output passes)
  perview  : (--views K > 1, one graph) K single-graph depths calls, one per view (seed + k), what a views x depths call replaces
  depths   : one ops.approximate_cholesky_depths (with views=K and node_ptr for a batch)
Graphs: ba1m (BA(1M, 10)), arxiv (BA(169343, 7), ogbn-arxiv's size), c5 (bench config 5: a node_ptr batch of 1024 x BA(4096, 8)).
Prints one JSON line per (graph, order, configuration) with the median wall time of a call (host clock around work that ends in the
call's own device synchronisation) and the last call's `last_stats`.  Every configuration runs in a fresh child process under a time
limit of its own.  --check compares every snapshot of the depths call with the CPU oracle once (not timed; on c5 the first and last
graph of every view); a mismatch ends the run with exit status 1.

  python tools/depths_latency.py --check
  python tools/depths_latency.py --check --views 2 --graphs ba1m,c5 --orders random
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ORDERS = {"degree": ("degree", "asc"), "random": ("random", "asc")}
GRAPHS = {"ba1m": (1000000, 10, 1), "arxiv": (169343, 7, 1), "c5": (4096, 8, 1024)}   # (nodes per graph, m, graphs)


def child(args):
    import numpy as np
    import torch
    from rlap_amd import graphs, ops
    o_v, o_n = ORDERS[args.order]
    n, m, G = GRAPHS[args.graph]
    K = args.views
    ts = [n // 8, n // 4, n // 2]
    e1 = graphs.barabasi_albert(n, m, 1)
    ei_cpu = torch.cat([e1 + g * n for g in range(G)], dim=1) if G > 1 else e1   # (c5: bench.py's batch, every graph alike)
    N = G * n
    node_ptr = [g * n for g in range(G + 1)] if G > 1 else None
    ei = ei_cpu.cuda()
    seed = 1234
    batched = K > 1 or G > 1

    def run():
        if args.config == "separate":
            if not batched:
                return [ops.approximate_cholesky(ei, None, n, t, o_v, o_n, seed=seed, return_device="same") for t in ts]
            return [ops.approximate_cholesky_views(ei, None, N, [t] * K, o_v, o_n, node_ptr=node_ptr, seed=seed) for t in ts]
        if args.config == "deepest":
            if not batched:
                return ops.approximate_cholesky(ei, None, n, ts[-1], o_v, o_n, seed=seed, return_device="same")
            return ops.approximate_cholesky_views(ei, None, N, [ts[-1]] * K, o_v, o_n, node_ptr=node_ptr, seed=seed)
        if args.config == "perview":
            assert G == 1, "perview: one graph"
            return [ops.approximate_cholesky_depths(ei, None, n, ts, o_v, o_n, seed=seed + k) for k in range(K)]
        if not batched:
            return ops.approximate_cholesky_depths(ei, None, n, ts, o_v, o_n, seed=seed)
        return ops.approximate_cholesky_depths(ei, None, N, ts, o_v, o_n, node_ptr=node_ptr, views=K, seed=seed)

    for _ in range(args.warmup):
        run()
    times = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    rec = {"graph": args.graph, "config": args.config, "order": f"{o_v}/{o_n}", "nodes": n, "m": m, "graphs": G, "views": K,
           "num_remove": ts, "ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_all": [round(x, 3) for x in times],
           "last_stats": ops.last_stats}
    if args.check and args.config == "depths":
        import oracle
        rng = np.random.RandomState(0)
        perm = np.concatenate([rng.permutation(n) for _ in range(K * G)]) if o_v == "random" else None
        p_t = torch.from_numpy(perm) if perm is not None else None
        if batched:
            sc, ptr = ops.approximate_cholesky_depths(ei, None, N, ts, o_v, o_n, node_ptr=node_ptr, views=K, seed=seed, perm=p_t)
        else:
            sc, ptr = ops.approximate_cholesky_depths(ei, None, n, ts, o_v, o_n, seed=seed, perm=p_t)
        sc = sc.cpu().numpy()
        ok, checked = True, 0
        e_np = e1.numpy()
        for d, t in enumerate(ts):
            for k in range(K):
                for g in sorted({0, G - 1}):
                    j = k * G + g
                    i = (d * K + k) * G + g
                    pk = None if perm is None else perm[j * n:(j + 1) * n]
                    ref = oracle.approximate_cholesky(e_np, None, n, t, o_v, o_n, perm=pk, shuffle_seed=seed + j)
                    v = sc[int(ptr[i]):int(ptr[i + 1])].copy()
                    v[:, :2] -= g * n
                    ok = ok and v.shape == ref.shape and bool(np.array_equal(v, ref))
                    checked += 1
        rec["oracle_bit_exact"] = ok
        rec["oracle_snapshots_checked"] = checked
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ba1m,arxiv")
    ap.add_argument("--orders", default="degree,random")
    ap.add_argument("--configs", default="separate,deepest,perview,depths")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per configuration (child process)")
    ap.add_argument("--check", action="store_true", help="compare the depths call with the CPU oracle once")
    ap.add_argument("--views", type=int, default=1, help="K views of every graph (perview: one graph only)")
    ap.add_argument("--config", help=argparse.SUPPRESS)
    ap.add_argument("--order", help=argparse.SUPPRESS)
    ap.add_argument("--graph", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.config:
        return child(args)
    for graph in args.graphs.split(","):
        for order in args.orders.split(","):
            for config in args.configs.split(","):
                if config == "perview" and (args.views < 2 or GRAPHS[graph][2] > 1):
                    continue
                cmd = [sys.executable, os.path.abspath(__file__), "--graph", graph, "--config", config, "--order", order,
                       "--warmup", str(args.warmup), "--repeat", str(args.repeat), "--views", str(args.views)] + (["--check"] if args.check else [])
                try:
                    p = subprocess.run(cmd, timeout=args.timeout, capture_output=True, text=True)
                except subprocess.TimeoutExpired:
                    print(json.dumps({"graph": graph, "config": config, "order": order, "error": f"timeout after {args.timeout} s"}), flush=True)
                    return 1
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
                if p.returncode != 0 or not lines:
                    print(json.dumps({"graph": graph, "config": config, "order": order, "error": f"exit {p.returncode}",
                                      "stderr": p.stderr[-2000:]}), flush=True)
                    return 1   # a failed GPU child ends the run: nothing more is started on the device
                print(lines[-1], flush=True)
                if json.loads(lines[-1]).get("oracle_bit_exact") is False:
                    return 1   # (--check: a snapshot differs from the oracle)
    return 0


if __name__ == "__main__":
    sys.exit(main())
