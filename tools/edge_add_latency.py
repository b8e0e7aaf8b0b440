"""ops.add_edges against a torch restatement of the reference's lines on the same device and tensors.  K = 2 views at
ratios (0.3, 0.4) -- one call here, two `augment` calls of the restatement, as the training scripts make them -- and one view, on
BA(1M, 10) and on the disjoint union of the batch of bench config 5 (1,024 BA(4096, 8) graphs), each graph once in coalesced order
(sorted by (source, target)) and once shuffled, coalesced and not.  The restatement of scripts/augmentor_benchmarks.py:44-54:
torch.randint, torch.cat, the key source * N + target and torch.unique(sorted=True, return_counts=True), which stands in for
sort_edge_index + coalesce: torch_sparse is not assumed.  Medians of 5 after a warm-up, host clock around a synchronise; the five
times are printed too.  Prints one JSON line per (graph, order, coalesce) (and appends it to --out).  `merge_bytes` is what the two
passes of the merge kernel must move at least: every key of A and of B_k read in both passes, a sum per key of A and a count per key
of B_k read and 24 bytes written per row in the second; the kernel's own time comes from a kernel trace of a --no-torch run and is
set against 8 TB/s in DESIGN 4.22.  Needs an MI355X; reads nothing outside the repository.

    python tools/edge_add_latency.py
    python tools/edge_add_latency.py --graphs ba --orders shuffled --modes coalesce --no-torch --no-one-view   # for a kernel trace
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
RATIOS = (0.3, 0.4)


def make(name):
    """(edge_index sorted by (source, target), N): the generator's graphs are symmetric and sorted by (target, source)."""
    if name == "ba":
        ei = graphs.barabasi_albert(1_000_000, 10, 1)
        return ei.flip(0).contiguous().cuda(), 1_000_000
    parts = [graphs.barabasi_albert(4096, 8, 1 + g).flip(0) + 4096 * g for g in range(1024)]
    return torch.cat(parts, 1).contiguous().cuda(), 4096 * 1024


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
def t_add_edge(ei, n, ratio, coalesce):
    num_add = int(ei.shape[1] * ratio)
    new = torch.randint(0, n - 1, size=(2, num_add), device=ei.device)
    cat = torch.cat([ei, new], dim=1)
    if not coalesce:
        return cat
    key, _ = torch.unique(cat[0] * n + cat[1], sorted=True, return_counts=True)
    return torch.stack([key // n, key % n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ba,c5")
    ap.add_argument("--orders", default="coalesced,shuffled")
    ap.add_argument("--modes", default="coalesce,plain")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--no-one-view", action="store_true", help="leave out the one-view calls (a kernel trace of K = 2 calls alone)")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    fh = open(args.out, "a") if args.out else None
    for gname in args.graphs.split(","):
        base, n = make(gname)
        E = int(base.shape[1])
        for order in args.orders.split(","):
            ei = base if order == "coalesced" else base[:, torch.randperm(E, generator=torch.Generator().manual_seed(1)).cuda()].contiguous()
            for mode in args.modes.split(","):
                coalesce = mode == "coalesce"
                rec = {"graph": gname, "N": n, "E": E, "order": order, "coalesce": coalesce, "K": 2, "ratios": list(RATIOS)}
                t, ts, res = timed(lambda: ops.add_edges(ei, None, n, list(RATIOS), 1, coalesce), args.reps)
                st = dict(ops.last_stats)
                M = int(res[0].shape[0])
                rec.update({"call_ms": round(t, 3), "call_runs_ms": ts, "rows": M, **{k: st[k] for k in ("added", "input_distinct", "input_sorted", "sorts",
                                                                                                      "launches", "host_syncs", "arena_bytes")}})
                del res
                if coalesce:
                    added, aptr = ops.add_edges(ei, None, n, list(RATIOS), 1, True, return_added=True)[2:]
                    a = aptr.tolist()
                    n_b = [int(torch.unique(added[a[k]:a[k + 1], 0] * n + added[a[k]:a[k + 1], 1]).numel()) for k in range(2)]
                    n_a = st["input_distinct"]
                    rec["merge_bytes"] = sum(2 * 8 * (n_a + b) + 8 * n_a + 4 * b for b in n_b) + 24 * M
                    del added
                if not args.no_one_view:
                    t1, ts1, _ = timed(lambda: ops.add_edges(ei, None, n, RATIOS[0], 1, coalesce), args.reps)
                    rec.update({"one_view_ms": round(t1, 3), "one_view_runs_ms": ts1})
                if not args.no_torch:
                    tt, tst, got = timed(lambda: [t_add_edge(ei, n, r, coalesce) for r in RATIOS], args.reps)
                    rec.update({"torch_two_augments_ms": round(tt, 3), "torch_runs_ms": tst, "torch_over_call": round(tt / t, 3),
                                "torch_rows": int(sum(g.shape[1] for g in got))})
                    del got
                line = json.dumps(rec)
                print(line, flush=True)
                if fh is not None:
                    fh.write(line + "\n")
                    fh.flush()
                torch.cuda.empty_cache()
            del ei
        del base
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
