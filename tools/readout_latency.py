"""ops.graph_readout against the same readout in torch on the same tensors and the same device.  The torch readouts
are what a graph-level step does today after every layer: per layer torch.zeros(G, F).index_add_(0, batch, z) -- global_add_pool --
and torch.segment_reduce(z, "sum", lengths=) where this torch has it.  Forward, and forward + backward (a gradient of ones-like
random values through the readout back to z).  float32 features.  Medians of 5 after a warm-up, host clock around a synchronise;
the five times are printed too.  Per shape: the time, the algorithmic bytes (L N F sizeof read once) over the time, and that rate as
a fraction of 8 TB/s.  Prints one JSON line per shape (and appends it to --out).  Needs an MI355X; reads nothing outside the
repository.

  c5    : the batch of bench config 5, 1,024 graphs of 4,096 nodes (N = 4,194,304), L = 3, F = 64 and 256
  loader: 128 graphs of 10 to 60 nodes, L = 2, F = 32 (the DataLoader(batch_size=128) shape of scripts/graph_shared.py)
  one   : one graph of 1,048,576 nodes, L = 1, F = 256
    python tools/readout_latency.py
    python tools/readout_latency.py --shapes c5 --features 64 --no-torch     # the calls alone (for rocprofv3 --kernel-trace --stats)
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

from rlap_amd import ops  # noqa: E402

PEAK = 8.0e12   # bytes per second, the HBM specification


def shapes():
    g = torch.Generator().manual_seed(1)
    loader = torch.randint(10, 61, (128,), generator=g).tolist()
    return {
        "c5": ([4096] * 1024, 3, (64, 256)),
        "loader": (loader, 2, (32,)),
        "one": ([1 << 20], 1, (256,)),
    }


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


def figures(rec, key, t, ts, nbytes):
    rate = nbytes / (t * 1e-3)
    rec.update({f"{key}_ms": round(t, 3), f"{key}_runs_ms": ts, f"{key}_bytes_per_s": round(rate, 1), f"{key}_of_8TBs": round(rate / PEAK, 4)})


def run(name, sizes, L, F, args, fh):
    G, N = len(sizes), sum(sizes)
    node_ptr = [0]
    for s in sizes:
        node_ptr.append(node_ptr[-1] + s)
    table = ops.GraphTable(node_ptr, N)
    lengths = torch.tensor(sizes, dtype=torch.int64, device="cuda")
    batch = torch.repeat_interleave(torch.arange(G, device="cuda"), lengths)
    gen = torch.Generator(device="cuda").manual_seed(F)
    x = torch.randn(L, N, F, dtype=torch.float32, device="cuda", generator=gen)
    gy = torch.randn(L, G, F, dtype=torch.float32, device="cuda", generator=gen)
    nbytes = L * N * F * 4
    rec = {"shape": name, "N": N, "G": G, "L": L, "F": F, "algorithmic_bytes": nbytes}

    def backward_of(fn):
        def both():
            z = x.detach().requires_grad_(True)
            fn(z).backward(gy)
            return z.grad
        return both

    t, ts, y = timed(lambda: ops.graph_readout(x, table), args.reps)
    figures(rec, "forward", t, ts, nbytes)
    st = dict(ops.last_stats)
    rec.update({"chunks": st["chunks"], "chunked_graphs": st["chunked_graphs"], "host_syncs": st["host_syncs"], "arena_bytes": st["arena_bytes"]})
    rec["repeats_bit_for_bit"] = bool(torch.equal(y, ops.graph_readout(x, table)))
    t2, ts2, gx = timed(backward_of(lambda z: ops.graph_readout(z, table)), args.reps)
    figures(rec, "forward_backward", t2, ts2, nbytes)
    rec["backward_is_the_gather"] = bool(torch.equal(gx[0, :: max(N // 4096, 1)], gy[0][batch[:: max(N // 4096, 1)]]))
    del gx
    if not args.no_torch:
        def index_add(z):
            return torch.stack([torch.zeros(G, F, dtype=z.dtype, device=z.device).index_add_(0, batch, z[l]) for l in range(L)])
        tt, tst, want = timed(lambda: index_add(x), args.reps)
        figures(rec, "torch_index_add", tt, tst, nbytes)
        rec.update({"torch_index_add_over_call": round(tt / t, 3), "max_abs_diff_to_index_add": float((y - want).abs().max()),
                    "max_abs_index_add": float(want.abs().max()), "index_add_repeats_bit_for_bit": bool(torch.equal(want, index_add(x)))})
        del want
        tt2, tst2, _ = timed(backward_of(index_add), args.reps)
        figures(rec, "torch_index_add_forward_backward", tt2, tst2, nbytes)
        rec["torch_index_add_forward_backward_over_call"] = round(tt2 / t2, 3)
        try:
            def seg(z):
                return torch.stack([torch.segment_reduce(z[l], "sum", lengths=lengths, axis=0, unsafe=True) for l in range(L)])
            ts_, tss, got = timed(lambda: seg(x), args.reps)
            figures(rec, "torch_segment_reduce", ts_, tss, nbytes)
            rec.update({"torch_segment_reduce_over_call": round(ts_ / t, 3), "max_abs_diff_to_segment_reduce": float((y - got).abs().max())})
            del got
            ts2_, tss2, _ = timed(backward_of(seg), args.reps)
            figures(rec, "torch_segment_reduce_forward_backward", ts2_, tss2, nbytes)
            rec["torch_segment_reduce_forward_backward_over_call"] = round(ts2_ / t2, 3)
        except Exception as exc:   # (not every torch build has it on the device)
            rec["torch_segment_reduce_ms"] = f"not available: {type(exc).__name__}: {exc}"[:200]
    line = json.dumps(rec)
    print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del x, gy, y
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="loader,one,c5")
    ap.add_argument("--features", default=None, help="comma-separated F values instead of the shape's own")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    fh = open(args.out, "a") if args.out else None
    all_shapes = shapes()
    for name in args.shapes.split(","):
        sizes, L, feats = all_shapes[name]
        for F in ([int(f) for f in args.features.split(",")] if args.features else feats):
            run(name, sizes, L, F, args, fh)


if __name__ == "__main__":
    main()
