"""Latency of K views of one graph, three ways, for the same graph and seeds:
  separate : K calls of ops.approximate_cholesky (seed + k)
  union    : one ops.approximate_cholesky_batched on the hand-built K-fold disjoint union (graphs.batch_disjoint)
  views    : one ops.approximate_cholesky_views
Prints one JSON line per (configuration, order) with the median wall time of a call (host clock around work that ends in the
call's own device synchronisation) and the last call's `last_stats`.  Every configuration runs in a fresh child process under a
time limit of its own.  --check compares each view of the views call with the CPU oracle once (not timed).

  python tools/views_latency.py --nodes 1000000 --m 10 --k 2 --check
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


def child(args):
    import numpy as np
    import torch
    from rlap_amd import graphs, ops
    o_v, o_n = ORDERS[args.order]
    n, K = args.nodes, args.k
    t = int(args.frac * n)
    ei_cpu = graphs.barabasi_albert(n, args.m, 1)
    ei = ei_cpu.cuda()
    seed = 1234
    if args.config == "union":
        big, node_ptr = graphs.batch_disjoint([ei_cpu] * K, [n] * K)
        big = big.cuda()

    def run():
        if args.config == "separate":
            return [ops.approximate_cholesky(ei, None, n, t, o_v, o_n, seed=seed + k, return_device="same") for k in range(K)]
        if args.config == "union":
            return ops.approximate_cholesky_batched(big, None, node_ptr, [t] * K, o_v, o_n, seed=seed)
        return ops.approximate_cholesky_views(ei, None, n, [t] * K, o_v, o_n, seed=seed)

    for _ in range(args.warmup):
        run()
    times = []
    for _ in range(args.repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    rec = {"config": args.config, "order": f"{o_v}/{o_n}", "nodes": n, "m": args.m, "k": K, "num_remove": t,
           "ms_median": float(np.median(times)), "ms_min": float(np.min(times)), "ms_all": [round(x, 3) for x in times],
           "last_stats": ops.last_stats}
    if args.check and args.config == "views":
        import oracle
        perms = [np.random.RandomState(k).permutation(n) for k in range(K)] if o_v == "random" else None
        sc, ptr = ops.approximate_cholesky_views(ei, None, n, [t] * K, o_v, o_n, seed=seed,
                                                 perm=torch.from_numpy(np.concatenate(perms)) if perms else None)
        sc = sc.cpu().numpy()
        ok = True
        for k in range(K):
            ref = oracle.approximate_cholesky(ei_cpu.numpy(), None, n, t, o_v, o_n, perm=perms[k] if perms else None, shuffle_seed=seed + k)
            v = sc[int(ptr[k]):int(ptr[k + 1])]
            ok = ok and v.shape == ref.shape and bool(np.array_equal(v, ref))
        rec["oracle_bit_exact"] = ok
    print(json.dumps(rec), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--frac", type=float, default=0.5)
    ap.add_argument("--orders", default="degree,random")
    ap.add_argument("--configs", default="separate,union,views")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=600, help="seconds per configuration (child process)")
    ap.add_argument("--check", action="store_true", help="compare the views call with the CPU oracle once")
    ap.add_argument("--config", help=argparse.SUPPRESS)
    ap.add_argument("--order", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.config:
        return child(args)
    for order in args.orders.split(","):
        for config in args.configs.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--config", config, "--order", order, "--nodes", str(args.nodes),
                   "--m", str(args.m), "--k", str(args.k), "--frac", str(args.frac), "--warmup", str(args.warmup),
                   "--repeat", str(args.repeat)] + (["--check"] if args.check else [])
            try:
                p = subprocess.run(cmd, timeout=args.timeout, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                print(json.dumps({"config": config, "order": order, "error": f"timeout after {args.timeout} s"}), flush=True)
                return 1
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                print(json.dumps({"config": config, "order": order, "error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]}), flush=True)
                return 1   # a failed GPU child ends the run: nothing more is started on the device
            print(lines[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
