"""Latency of K nested Schur complements of one graph, three ways, for the same graph, seed and depths [N/8, N/4, N/2]:
  separate : K calls of ops.approximate_cholesky, one per depth
  deepest  : the one call at the deepest depth (what the depths call should cost, plus K-1 output passes)
  depths   : one ops.approximate_cholesky_depths
Prints one JSON line per (graph, order, configuration) with the median wall time of a call (host clock around work that ends in the
call's own device synchronisation) and the last call's `last_stats`.  Every configuration runs in a fresh child process under a time
limit of its own.  --check compares each snapshot of the depths call with the CPU oracle once (not timed); a mismatch ends the run
with exit status 1.

  python tools/depths_latency.py --check
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
GRAPHS = {"ba1m": (1000000, 10), "arxiv": (169343, 7)}   # BA(1M, 10); BA(169343, 7), ogbn-arxiv's size


def child(args):
    import numpy as np
    import torch
    from rlap_amd import graphs, ops
    o_v, o_n = ORDERS[args.order]
    n, m = GRAPHS[args.graph]
    ts = [n // 8, n // 4, n // 2]
    ei_cpu = graphs.barabasi_albert(n, m, 1)
    ei = ei_cpu.cuda()
    seed = 1234

    def run():
        if args.config == "separate":
            return [ops.approximate_cholesky(ei, None, n, t, o_v, o_n, seed=seed, return_device="same") for t in ts]
        if args.config == "deepest":
            return ops.approximate_cholesky(ei, None, n, ts[-1], o_v, o_n, seed=seed, return_device="same")
        return ops.approximate_cholesky_depths(ei, None, n, ts, o_v, o_n, seed=seed)

    for _ in range(args.warmup):
        run()
    times = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    rec = {"graph": args.graph, "config": args.config, "order": f"{o_v}/{o_n}", "nodes": n, "m": m, "num_remove": ts,
           "ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_all": [round(x, 3) for x in times],
           "last_stats": ops.last_stats}
    if args.check and args.config == "depths":
        import oracle
        perm = np.random.RandomState(0).permutation(n) if o_v == "random" else None
        sc, ptr = ops.approximate_cholesky_depths(ei, None, n, ts, o_v, o_n, seed=seed,
                                                  perm=torch.from_numpy(perm) if perm is not None else None)
        sc = sc.cpu().numpy()
        ok = True
        for k, t in enumerate(ts):
            ref = oracle.approximate_cholesky(ei_cpu.numpy(), None, n, t, o_v, o_n, perm=perm, shuffle_seed=seed)
            v = sc[int(ptr[k]):int(ptr[k + 1])]
            ok = ok and v.shape == ref.shape and bool(np.array_equal(v, ref))
        rec["oracle_bit_exact"] = ok
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ba1m,arxiv")
    ap.add_argument("--orders", default="degree,random")
    ap.add_argument("--configs", default="separate,deepest,depths")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per configuration (child process)")
    ap.add_argument("--check", action="store_true", help="compare the depths call with the CPU oracle once")
    ap.add_argument("--config", help=argparse.SUPPRESS)
    ap.add_argument("--order", help=argparse.SUPPRESS)
    ap.add_argument("--graph", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.config:
        return child(args)
    for graph in args.graphs.split(","):
        for order in args.orders.split(","):
            for config in args.configs.split(","):
                cmd = [sys.executable, os.path.abspath(__file__), "--graph", graph, "--config", config, "--order", order,
                       "--warmup", str(args.warmup), "--repeat", str(args.repeat)] + (["--check"] if args.check else [])
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
