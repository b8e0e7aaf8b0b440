"""ops.snapshot_subgraph against the torch formulation (per segment: torch.unique, isin, boolean mask, searchsorted) on the same
inputs and the same device.  Medians of 5 after a warm-up, host clock around a synchronise; the five times are printed too, so a
difference can be held against the run-to-run spread.  Prints one JSON line per case (and appends them to --out FILE when given).

    python tools/subgraph_latency.py                      # both cases below
    python tools/subgraph_latency.py --case depths        # BA(1M, 10), depths [N/8, N/4, N/2], views=2, random: nodes=None, relabel
    python tools/subgraph_latency.py --case ppr           # snapshot_ppr result of BA(34,493, 7) frac 0.5: remove_self_loops, then
                                                          # the subgraph of a batch of 8,192 nodes
    python tools/subgraph_latency.py --case depths --n 200000 --m 8 --no-torch     # another size; the call alone (for a profiler)
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


def torch_formulation(sc, ptr, nodes_of=None, relabel=False, remove_self_loops=False):
    p = torch.as_tensor(ptr).tolist()
    outs, idss = [], []
    for s in range(len(p) - 1):
        part = sc[p[s]:p[s + 1]]
        i, j = part[:, 0].long(), part[:, 1].long()
        if nodes_of is None:
            src = part[:, :2].long()
            ids = torch.unique(src[i != j] if remove_self_loops else src)
        else:
            ids = torch.unique(nodes_of(s))
        keep = torch.isin(i, ids) & torch.isin(j, ids)
        if remove_self_loops:
            keep &= i != j
        out = part[keep]
        if relabel:
            out = torch.stack([torch.searchsorted(ids, i[keep]).double(), torch.searchsorted(ids, j[keep]).double(), out[:, 2]], 1)
        outs.append(out)
        idss.append(ids)
    return torch.cat(outs), torch.cat(idss)


def emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def compare(rec, name, call, ref, reps, no_torch):
    """Times `call` (-> out, optr, ids, iptr) and `ref` (-> out, ids) into rec[name + ...]; both must give the same tensors."""
    t, ts, got = timed(call, reps)
    st = dict(ops.last_stats)
    rec.update({name + "_ms": round(t, 3), name + "_runs_ms": ts, name + "_rows_kept": st["rows_kept"], name + "_ids": st["ids_written"],
                name + "_host_syncs": st["host_syncs"], name + "_arena_bytes": st["arena_bytes"]})
    if no_torch:
        return got
    try:
        t_ref, ts_ref, want = timed(ref, reps)
        rec.update({name + "_torch_ms": round(t_ref, 3), name + "_torch_runs_ms": ts_ref, name + "_torch_over_call": round(t_ref / t, 3),
                    name + "_same": bool(torch.equal(got[0], want[0]) and torch.equal(got[2], want[1]))})
        del want
    except RuntimeError as e:   # (the torch path's own failure, an allocation say, is a result too)
        rec[name + "_torch_error"] = str(e).splitlines()[0][:160]
    torch.cuda.empty_cache()
    return got


def case_depths(args, fh):
    n, m = args.n, args.m
    ei = graphs.barabasi_albert(n, m, 1).cuda()
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, [n // 8, n // 4, n // 2], "random", "asc", views=2, seed=1, return_device="same")
    del ei
    rows = int(sc.shape[0])
    rec = {"case": "depths", "n": n, "m": m, "segments": int(ptr.numel() - 1), "rows": rows}
    got = compare(rec, "relabel", lambda: ops.snapshot_subgraph(sc, ptr, n, relabel=True),
                  lambda: torch_formulation(sc, ptr, relabel=True), args.reps, args.no_torch)
    # algorithmic bytes of the two filter passes: every row read twice, the kept rows written once, 24 B each
    rec["filter_bytes"] = 24 * (2 * rows + int(got[0].shape[0]))
    emit(rec, fh)


def case_ppr(args, fh):
    n = 34493
    ei = graphs.barabasi_albert(n, 7, 1).cuda()
    sc = ops.approximate_cholesky(ei, None, n, n // 2, "random", "asc", seed=1, return_device="same")
    out, pptr = ops.snapshot_ppr(sc, [0, sc.shape[0]], n)
    rec = {"case": "ppr", "n": n, "m": 7, "frac": 0.5, "rows": int(out.shape[0])}
    got = compare(rec, "node_set", lambda: ops.snapshot_subgraph(out, pptr, n, remove_self_loops=True),
                  lambda: torch_formulation(out, pptr, remove_self_loops=True), args.reps, args.no_torch)
    ids = got[2]
    batch = ids[torch.randperm(ids.numel(), generator=torch.Generator().manual_seed(1))[:8192].cuda()]
    compare(rec, "batch", lambda: ops.snapshot_subgraph(out, pptr, n, nodes=batch),
            lambda: torch_formulation(out, pptr, lambda s: batch), args.reps, args.no_torch)
    emit(rec, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["depths", "ppr", "all"], default="all")
    ap.add_argument("--n", type=int, default=1_000_000, help="nodes of the BA graph of the depths case")
    ap.add_argument("--m", type=int, default=10, help="its attachment count")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the call alone")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    fh = open(args.out, "a") if args.out else None
    if args.case in ("ppr", "all"):
        case_ppr(args, fh)
    if args.case in ("depths", "all"):
        case_depths(args, fh)


if __name__ == "__main__":
    main()
