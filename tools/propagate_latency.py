"""ops.snapshot_propagate against the same product in torch on the same tensors and the same device.  The torch
product is what a GCNConv(normalize=False) does with the list of ops.snapshot_gcn_norm: per layer (the snapshots of one layer are one
batch over disjoint ids) torch.zeros(N, F).index_add_(0, dst, val[:, None] * x[src]); the list itself is built outside the timed
span, and the time of building it (ops.snapshot_gcn_norm) is reported beside it, since the call under test needs no list.  Where
this ROCm supports it, torch.sparse.mm on a CSR matrix built outside the timed span is timed too.  float32 features, F = 64 and 256.
Medians of 5 after a warm-up, host clock around a synchronise; the five times are printed too.  Prints one JSON line per graph and F
(and appends it to --out).

  ba1m : BA(1M, 10), depths [N/8, N/4, N/2], views=2, random (6 snapshots, 6 layers)
  c5   : bench config 5, a node_ptr batch of 1024 x BA(4096, 8), depths [n/8, n/4, n/2] (3,072 snapshots, 3 layers)
    python tools/propagate_latency.py --graphs ba1m,c5
    python tools/propagate_latency.py --graphs ba1m --features 256 --no-torch     # the calls alone (for rocprofv3 --kernel-trace --stats)
    python tools/propagate_latency.py --plan --no-torch                           # and the same products over a propagation plan
--plan adds, next to the figures above: the time of ops.snapshot_plan (both directions), the planned forward product and
the planned forward + transposed pair, the plan's bytes, the algorithmic bytes of k_pl_rows and the calls after which the plan has paid
for itself, build time / (unplanned forward - planned forward).  --plan-only leaves the unplanned calls out (a profile of the planned
kernels alone; also what runs against a library without the plan exports when it is absent).
--edges times the plans of rows in any order instead: ops.edge_plan of the BA(1M, 10) input graph itself (20 M directed
rows) against the torch pipeline for the same structure on the same tensors -- the gcn_norm formulation of 4.10 plus a stable sort by
target into CSR arrays -- and ops.edge_list_plan of the six-snapshot elimination result against ops.snapshot_plan of the same rows
(rlap_plan.hip is the parent's, unchanged), with the plan bytes and the planned products of both.
    python tools/propagate_latency.py --edges --features 64
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


def torch_product(ei, val, bounds, N, x, transpose=False):
    """[y_l] per layer from the list of ops.snapshot_gcn_norm."""
    out = []
    for a, b in bounds:
        src, dst = (ei[1, a:b], ei[0, a:b]) if transpose else (ei[0, a:b], ei[1, a:b])
        out.append(torch.zeros(N, x.shape[1], dtype=x.dtype, device=x.device).index_add_(0, dst, val[a:b, None] * x[src]))
    return out


def run(name, F, args, fh):
    n, m, G, K = GRAPHS[name]
    e1 = graphs.barabasi_albert(n, m, 1)
    ei = (torch.cat([e1 + g * n for g in range(G)], dim=1) if G > 1 else e1).cuda()
    N = G * n
    node_ptr = [g * n for g in range(G + 1)] if G > 1 else None
    sc, ptr = ops.approximate_cholesky_depths(ei, None, N, [n // 8, n // 4, n // 2], "random", "asc", node_ptr=node_ptr, views=K, seed=1,
                                              return_device="same")
    del ei
    S = ptr.numel() - 1
    L = S // G
    rows = int(sc.shape[0])
    x = torch.randn(N, F, dtype=torch.float32, generator=torch.Generator().manual_seed(F)).cuda()
    rec = {"graph": name, "F": F, "snapshots": S, "layers": L, "rows": rows}
    if args.plan_only:
        plan_figures(rec, sc, ptr, N, node_ptr, x, L, F, None, None, args)
        emit(rec, fh)
        return
    t, ts, y = timed(lambda: ops.snapshot_propagate(sc, ptr, N, x, node_ptr=node_ptr), args.reps)
    st = dict(ops.last_stats)
    M = st["entries"]
    # algorithmic bytes of the main kernel (k_sp_rows): per entry the gathered row of x, the 24-byte row, rb and blk and two dis; y
    # written once.  Divide them by that kernel's time from a rocprofv3 --kernel-trace --stats run of this tool with --no-torch
    # for its achieved rate (the gathers are partly served from L2 and the Infinity Cache: a rate, not an HBM figure); divided by
    # the whole call, column pass and host synchronisation included, they give the call's rate below.
    sum_bytes = M * (4 * F + 24 + 4 + 4 + 16) + 4 * L * N * F
    rec.update({"forward_ms": round(t, 3), "forward_runs_ms": ts, "entries": M, "blocks": st["blocks"], "chunked_lists": st["chunked_lists"],
                "host_syncs": st["host_syncs"], "arena_bytes": st["arena_bytes"], "main_kernel_bytes": sum_bytes,
                "whole_call_bytes_per_s": round(sum_bytes / (t * 1e-3), 1)})

    def both():
        out = ops.snapshot_propagate(sc, ptr, N, x, node_ptr=node_ptr)
        return ops.snapshot_propagate(sc, ptr, N, out, node_ptr=node_ptr, transpose=True)
    t2, ts2, _ = timed(both, args.reps)
    rec.update({"forward_transpose_ms": round(t2, 3), "forward_transpose_runs_ms": ts2})
    if args.plan:
        plan_figures(rec, sc, ptr, N, node_ptr, x, L, F, t, y, args)
    if not args.no_torch:
        tl, tsl, (eidx, val, eptr) = timed(lambda: ops.snapshot_gcn_norm(sc, ptr, N, node_ptr=node_ptr), args.reps)
        e = eptr.tolist()
        bounds = [(e[l * G], e[(l + 1) * G]) for l in range(L)]
        tt, tst, want = timed(lambda: torch_product(eidx, val, bounds, N, x), args.reps)
        diff = max(float((y[l] - want[l]).abs().max()) for l in range(L))
        scale = max(float(want[l].abs().max()) for l in range(L))
        rec.update({"gcn_norm_ms": round(tl, 3), "torch_ms": round(tt, 3), "torch_runs_ms": tst, "torch_over_call": round(tt / t, 3),
                    "torch_with_list_over_call": round((tt + tl) / t, 3), "max_abs_diff_to_torch_f32": diff, "max_abs_torch": scale})

        def torch_both():
            out = torch_product(eidx, val, bounds, N, x)
            return [torch_product(eidx, val, [bounds[l]], N, out[l], transpose=True)[0] for l in range(L)]
        del want
        tt2, tst2, _ = timed(torch_both, args.reps)
        rec.update({"torch_forward_transpose_ms": round(tt2, 3), "torch_forward_transpose_runs_ms": tst2,
                    "torch_forward_transpose_over_call": round(tt2 / t2, 3)})
        try:   # CSR per layer, built outside the timed span (row = target)
            mats = [torch.sparse_coo_tensor(torch.stack([eidx[1, a:b], eidx[0, a:b]]), val[a:b], (N, N)).coalesce().to_sparse_csr()
                    for a, b in bounds]
            ts_, tss, got = timed(lambda: [torch.sparse.mm(mt, x) for mt in mats], args.reps)
            rec.update({"torch_csr_ms": round(ts_, 3), "torch_csr_runs_ms": tss, "torch_csr_over_call": round(ts_ / t, 3),
                        "max_abs_diff_to_csr_f32": max(float((y[l] - got[l]).abs().max()) for l in range(L))})
            del mats, got
        except Exception as exc:   # (not every ROCm build has the CSR product)
            rec["torch_csr_ms"] = f"not available: {type(exc).__name__}"
        del eidx, val
    emit(rec, fh)
    del sc, x, y
    torch.cuda.empty_cache()


def emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()


def plan_figures(rec, sc, ptr, N, node_ptr, x, L, F, unplanned_ms, y, args):
    """The planned products of the same input: build, forward, forward + transposed, bytes."""
    tb, tsb, plan = timed(lambda: ops.snapshot_plan(sc, ptr, N, node_ptr=node_ptr), args.reps)
    info = dict(plan.info)
    tp, tsp, yp = timed(lambda: plan.propagate(x), args.reps)
    syncs = ops.last_stats["host_syncs"]

    def both():
        return plan.propagate(plan.propagate(x), transpose=True)
    tp2, tsp2, _ = timed(both, args.reps)
    M = info["entries"]
    records = int(plan.desc.entries_forward)
    # algorithmic bytes of k_pl_rows: per record its 16 bytes and the gathered row of x; per (layer, id) two offsets (one new), the
    # loop coefficient and the loop's row of x (inside M); y written once
    rows_bytes = records * 16 + M * 4 * F + L * N * (8 + 8) + 4 * L * N * F
    rec.update({"plan_build_ms": round(tb, 3), "plan_build_runs_ms": tsb, "plan_bytes": plan.nbytes, "plan_entries": M,
                "plan_chunked_lists": [info["chunked_lists_forward"], info["chunked_lists_transposed"]],
                "planned_forward_ms": round(tp, 3), "planned_forward_runs_ms": tsp, "planned_forward_transpose_ms": round(tp2, 3),
                "planned_forward_transpose_runs_ms": tsp2, "planned_host_syncs": syncs, "plan_rows_kernel_bytes": rows_bytes,
                "planned_whole_call_bytes_per_s": round(rows_bytes / (tp * 1e-3), 1)})
    if unplanned_ms is not None:
        rec["planned_equals_unplanned"] = bool(torch.equal(yp, y))
        gain = unplanned_ms - tp
        rec["plan_pays_after_calls"] = round(tb / gain, 2) if gain > 0 else None
    del plan, yp


def torch_gcn_csr(ei, N):
    """The torch pipeline an edge plan replaces, forward direction: add_remaining_self_loops + gcn_norm (DESIGN 4.10's formulation,
    unit weights), then a stable sort by target into CSR arrays (crow, col, val)."""
    ar = torch.arange(N, device=ei.device)
    keep = ei[0] != ei[1]
    src, dst = torch.cat([ei[0][keep], ar]), torch.cat([ei[1][keep], ar])
    w = torch.ones(src.numel(), dtype=torch.float64, device=ei.device)
    deg = torch.zeros(N, dtype=torch.float64, device=ei.device).index_add_(0, dst, w)
    dis = deg.pow(-0.5)
    dis[dis == float("inf")] = 0.0
    val = dis[src] * w * dis[dst]
    order = torch.argsort(dst, stable=True)
    crow = torch.zeros(N + 1, dtype=torch.int64, device=ei.device)
    crow[1:] = torch.cumsum(torch.bincount(dst, minlength=N), 0)
    return crow, src[order], val[order]


def run_edges(F, args, fh):
    n, m, _, K = GRAPHS["ba1m"]
    ei = graphs.barabasi_albert(n, m, 1).cuda()
    x = torch.randn(n, F, dtype=torch.float32, generator=torch.Generator().manual_seed(F)).cuda()
    rec = {"graph": "ba1m input graph", "F": F, "rows": int(ei.shape[1])}
    tb, tsb, plan = timed(lambda: ops.edge_plan(ei, None, n), args.reps)
    rows = torch.empty((ei.shape[1], 3), dtype=torch.float64, device="cuda")
    rows[:, 0], rows[:, 1], rows[:, 2] = ei[0], ei[1], 1.0
    tl, tsl, _ = timed(lambda: ops.edge_list_plan(rows, [0, int(rows.shape[0])], n), args.reps)
    del rows
    tp, tsp, y = timed(lambda: plan.propagate(x), args.reps)
    tp2, tsp2, _ = timed(lambda: plan.propagate(plan.propagate(x), transpose=True), args.reps)
    rec.update({"edge_plan_ms": round(tb, 3), "edge_plan_runs_ms": tsb, "edge_list_plan_ms": round(tl, 3), "edge_list_plan_runs_ms": tsl,
                "plan_bytes": plan.nbytes, "planned_forward_ms": round(tp, 3), "planned_forward_runs_ms": tsp,
                "planned_forward_transpose_ms": round(tp2, 3), "planned_forward_transpose_runs_ms": tsp2})
    if not args.no_torch:
        tt, tst, (crow, col, val) = timed(lambda: torch_gcn_csr(ei, n), args.reps)
        want = torch.zeros(n, F, dtype=torch.float64, device="cuda").index_add_(
            0, torch.repeat_interleave(torch.arange(n, device="cuda"), crow[1:] - crow[:-1]), val[:, None] * x[col].double())
        rec.update({"torch_gcn_norm_csr_ms": round(tt, 3), "torch_gcn_norm_csr_runs_ms": tst, "torch_over_edge_plan": round(tt / tb, 3),
                    "max_abs_diff_to_torch": float((y[0].double() - want).abs().max())})
        del crow, col, val, want
    emit(rec, fh)
    del plan, y, ei
    torch.cuda.empty_cache()
    # the elimination result propagate_latency already uses: the same rows through both builds
    ei = graphs.barabasi_albert(n, m, 1).cuda()
    sc, ptr = ops.approximate_cholesky_depths(ei, None, n, [n // 8, n // 4, n // 2], "random", "asc", views=K, seed=1, return_device="same")
    del ei
    rec = {"graph": "ba1m elimination result", "F": F, "snapshots": ptr.numel() - 1, "rows": int(sc.shape[0])}
    ts_, tss, splan = timed(lambda: ops.snapshot_plan(sc, ptr, n), args.reps)
    te, tse, eplan = timed(lambda: ops.edge_list_plan(sc, ptr, n), args.reps)
    rec.update({"snapshot_plan_ms": round(ts_, 3), "snapshot_plan_runs_ms": tss, "edge_list_plan_ms": round(te, 3), "edge_list_plan_runs_ms": tse,
                "edge_over_snapshot_build": round(te / ts_, 3), "snapshot_plan_bytes": splan.nbytes, "edge_plan_bytes": eplan.nbytes})
    for name, pl in (("snapshot", splan), ("edge", eplan)):
        tp, tsp, y = timed(lambda: pl.propagate(x), args.reps)
        tp2, tsp2, _ = timed(lambda: pl.propagate(pl.propagate(x), transpose=True), args.reps)
        rec.update({f"{name}_planned_forward_ms": round(tp, 3), f"{name}_planned_forward_runs_ms": tsp,
                    f"{name}_planned_forward_transpose_ms": round(tp2, 3), f"{name}_planned_forward_transpose_runs_ms": tsp2})
    rec["products_equal"] = bool(torch.equal(splan.propagate(x), eplan.propagate(x))
                                 and torch.equal(splan.propagate(x, transpose=True), eplan.propagate(x, transpose=True)))
    emit(rec, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="ba1m,c5")
    ap.add_argument("--features", default="64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--plan", action="store_true", help="also build a propagation plan and time the planned products")
    ap.add_argument("--plan-only", action="store_true", help="the planned products alone")
    ap.add_argument("--edges", action="store_true", help="the plans of rows in any order (ops.edge_plan / edge_list_plan) instead")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    fh = open(args.out, "a") if args.out else None
    if args.edges:
        for F in args.features.split(","):
            run_edges(int(F), args, fh)
        return
    for g in args.graphs.split(","):
        for F in args.features.split(","):
            run(g, int(F), args, fh)


if __name__ == "__main__":
    main()
