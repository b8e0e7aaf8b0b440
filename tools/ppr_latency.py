"""Dense adapters.compute_ppr against ops.snapshot_ppr per snapshot, and the fraction sweep of scripts/rlap_ppr_edge_plots.py (one
depths call + one snapshot_ppr against five rLap calls + five dense diffusions).  Medians of 5 after a warm-up, host clock around a
synchronise.  Prints one JSON line per case (and appends them to --out FILE when given).

    python tools/ppr_latency.py                 # Cora / Coauthor-CS / Coauthor-Physics shapes, frac 0.1 and 0.5, and the sweeps
    python tools/ppr_latency.py --big           # BA(169,343, 7) at frac 0.5, sparse only (the dense working set is computed)
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

from rlap_amd import adapters, graphs, ops  # noqa: E402

SHAPES = [("cora", 2708, 2), ("coauthor_cs", 18333, 4), ("coauthor_physics", 34493, 7)]


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
    return statistics.median(ts), res


def dense_call(sc, n):
    ei = sc[:, :2].long().t()
    nodes = torch.unique(ei, sorted=True)
    rel = torch.full((n,), -1, dtype=torch.int64, device=ei.device)
    rel[nodes] = torch.arange(nodes.numel(), device=ei.device)
    return adapters.compute_ppr(rel[ei], sc[:, 2], nodes.numel())


def emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    fh = open(args.out, "a") if args.out else None
    cases = [("ogbn_arxiv_stand_in", 169343, 7)] if args.big else SHAPES
    fracs = (0.5,) if args.big else (0.1, 0.5)
    for name, n, mdeg in cases:
        ei = graphs.barabasi_albert(n, mdeg, 1).cuda()
        for frac in fracs:
            sc = ops.approximate_cholesky(ei, None, n, int(frac * n), "random", "asc", seed=1, return_device="same")
            ns = int(torch.unique(sc[:, :2].long()).numel())
            torch.cuda.reset_peak_memory_stats()
            t_sparse, (out, _) = timed(lambda: ops.snapshot_ppr(sc, [0, sc.shape[0]], n), args.reps)
            st = dict(ops.last_stats)
            rec = {"graph": name, "n": n, "m": mdeg, "frac": frac, "n_s": ns, "rows_s": int(sc.shape[0]), "ppr_rows": int(out.shape[0]),
                   "sparse_ms": round(t_sparse, 3), "steps": st["steps"], "small_tiles": st["small_tiles"],
                   "large_tiles": st["large_tiles"], "groups": st["groups"], "arena_bytes": st["arena_bytes"],
                   "host_syncs": st["host_syncs"], "output_retries": st["output_retries"], "first_cap": st["first_cap"],
                   "torch_peak_bytes": torch.cuda.max_memory_allocated()}
            dense_bytes = 5 * ns * ns * 8
            rec["dense_working_set_bytes"] = dense_bytes
            if not args.big and not args.no_dense:
                try:
                    t_dense, (di, dw) = timed(lambda: dense_call(sc, n), args.reps)
                    rec["dense_ms"] = round(t_dense, 3)
                    rec["dense_over_sparse"] = round(t_dense / t_sparse, 3)
                    rec["same_rows"] = bool(di.shape[1] == out.shape[0])
                    del di, dw
                except RuntimeError as e:   # (the dense path's own failure is a result too)
                    rec["dense_error"] = str(e).splitlines()[0][:160]
                torch.cuda.empty_cache()
            emit(rec, fh)
            del out
            torch.cuda.empty_cache()
        if args.big:
            continue
        # the sweep of scripts/rlap_ppr_edge_plots.py: fractions 0.1 .. 0.5
        fr = (0.1, 0.2, 0.3, 0.4, 0.5)
        x = torch.zeros((n, 1), device="cuda")

        def sparse_sweep():
            return adapters.rLapDepths(fr, o_v="random", seed=1).diffuse((x, ei, None))

        def dense_sweep():
            res = []
            for f in fr:
                aug = adapters.rLapPPRDiffusion(f, o_v="random", seed=1, use_cache=False)
                res.append(aug.augment((x, ei, None)))
            return res
        t_s, _ = timed(sparse_sweep, args.reps)
        st = dict(ops.last_stats)
        rec = {"graph": name, "n": n, "m": mdeg, "sweep": list(fr), "sparse_ms": round(t_s, 3), "host_syncs": st["host_syncs"],
               "output_retries": st["output_retries"], "arena_bytes": st["arena_bytes"]}
        if not args.no_dense:
            try:
                t_d, _ = timed(dense_sweep, args.reps)
                rec["dense_ms"] = round(t_d, 3)
                rec["dense_over_sparse"] = round(t_d / t_s, 3)
            except RuntimeError as e:
                rec["dense_error"] = str(e).splitlines()[0][:160]
        emit(rec, fh)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
