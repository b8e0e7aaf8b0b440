"""ops.snapshot_gcn_norm against the torch formulation on the same tensors and the same device: per snapshot the slice,
.long().t().contiguous(), add_remaining_self_loops (mask row != col, cat with arange), the degree index_add_, pow(-0.5) and the
gather-multiply -- in float32 with unit weights, as PyG's gcn_norm runs it for edge_weight=None.  And the conversion alone
(normalize=False, add_self_loops=False) against the bare sc[:, :2].long().t().contiguous() per snapshot.  Medians of 5 after a
warm-up, host clock around a synchronise; the five times are printed too.  Prints one JSON line per graph (and appends it to --out).

  ba1m : BA(1M, 10), depths [N/8, N/4, N/2], views=2, random (6 snapshots)
  c5   : bench config 5, a node_ptr batch of 1024 x BA(4096, 8), depths [n/8, n/4, n/2] (3,072 snapshots)
    python tools/gcn_norm_latency.py --graphs ba1m,c5
    python tools/gcn_norm_latency.py --graphs ba1m --no-torch        # the calls alone (for rocprofv3 --kernel-trace --stats)
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

GRAPHS = {"ba1m": (1000000, 10, 1, 2), "c5": (4096, 8, 1024, 1)}   # (nodes per graph, m, graphs, views)


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


def torch_formulation(sc, p, ranges):
    """[(edge_index, weight)] per snapshot: what the training script does today with every view."""
    out = []
    for s in range(len(p) - 1):
        lo, hi = ranges[s]
        ei = sc[p[s]:p[s + 1], :2].long().t().contiguous()
        mask = ei[0] != ei[1]
        ar = torch.arange(lo, hi, device=sc.device)
        ei = torch.cat([ei[:, mask], torch.stack([ar, ar])], 1)
        w = torch.ones(ei.shape[1], dtype=torch.float32, device=sc.device)
        deg = torch.zeros(hi, dtype=torch.float32, device=sc.device).index_add_(0, ei[1], w)
        dis = deg.pow(-0.5)
        dis.masked_fill_(dis == float("inf"), 0.0)
        out.append((ei, dis[ei[0]] * w * dis[ei[1]]))
    return out


def torch_conversion(sc, p):
    return [sc[p[s]:p[s + 1], :2].long().t().contiguous() for s in range(len(p) - 1)]


def run(name, args, fh):
    n, m, G, K = GRAPHS[name]
    e1 = graphs.barabasi_albert(n, m, 1)
    ei = (torch.cat([e1 + g * n for g in range(G)], dim=1) if G > 1 else e1).cuda()
    N = G * n
    node_ptr = [g * n for g in range(G + 1)] if G > 1 else None
    sc, ptr = ops.approximate_cholesky_depths(ei, None, N, [n // 8, n // 4, n // 2], "random", "asc", node_ptr=node_ptr, views=K, seed=1,
                                              return_device="same")
    del ei
    p = ptr.tolist()
    S = len(p) - 1
    ranges = [((s % G) * n, (s % G + 1) * n) for s in range(S)]
    rows = int(sc.shape[0])
    rec = {"graph": name, "snapshots": S, "rows": rows}
    t, ts, got = timed(lambda: ops.snapshot_gcn_norm(sc, ptr, N, node_ptr=node_ptr), args.reps)
    st = dict(ops.last_stats)
    M = st["entries"]
    rec.update({"call_ms": round(t, 3), "call_runs_ms": ts, "entries": M, "loops_removed": st["loops_removed"],
                "host_syncs": st["host_syncs"], "arena_bytes": st["arena_bytes"],
                # algorithmic bytes of the emit pass: rows and rb read, src / dst / float32 val written
                "emit_bytes": 28 * rows + 20 * M})
    tc, tsc, conv = timed(lambda: ops.snapshot_gcn_norm(sc, ptr, N, node_ptr=node_ptr, normalize=False, add_self_loops=False), args.reps)
    rec.update({"convert_ms": round(tc, 3), "convert_runs_ms": tsc})
    if not args.no_torch:
        t_ref, ts_ref, want = timed(lambda: torch_formulation(sc, p, ranges), args.reps)
        e = got[2].tolist()
        same_ei = all(torch.equal(got[0][:, e[s]:e[s + 1]], want[s][0]) for s in range(S))
        rel = max(float(((got[1][e[s]:e[s + 1]] - want[s][1]).abs() / want[s][1].abs().clamp_min(1e-30)).max()) for s in range(S)
                  if e[s + 1] > e[s])
        rec.update({"torch_ms": round(t_ref, 3), "torch_runs_ms": ts_ref, "torch_over_call": round(t_ref / t, 3),
                    "same_edge_index": same_ei, "max_rel_diff_to_torch_f32": rel})
        del want
        t_cv, ts_cv, want = timed(lambda: torch_conversion(sc, p), args.reps)
        rec.update({"torch_convert_ms": round(t_cv, 3), "torch_convert_runs_ms": ts_cv, "torch_convert_over_call": round(t_cv / tc, 3),
                    "same_conversion": all(torch.equal(conv[0][:, p[s]:p[s + 1]], want[s]) for s in range(S))})
        del want
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del sc, got, conv
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ba1m,c5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    fh = open(args.out, "a") if args.out else None
    for g in args.graphs.split(","):
        run(g, args, fh)


if __name__ == "__main__":
    main()
