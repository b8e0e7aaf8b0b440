"""The sparse first layer (ops.feature_plan / FeaturePlan.linear) against torch on the same tensors and the same device:
every view's (x * keep[k]) @ W, forward and forward + backward (W requires a gradient; the upstream gradient is a fixed random
tensor), float32, K = 2 views, p = 0.3, Fout 256 and 512.  The datasets are not read: x is a seeded row-normalised bag-of-words
matrix at the reference's shapes -- `nz` distinct-or-colliding random columns a row set to 1, the row divided by its sum.

  cora    : 2,708 x 1,433, 18 non-zeros a row (Cora's 49,216 / 2,708)
  cs      : 18,333 x 6,805, --nz a row (default 32; the real density of Coauthor-CS was not available)
  physics : 34,493 x 8,415, --nz a row (default 32; the real density of Coauthor-Physics was not available)

Three sides, timed alternately in one run, rep by rep:
  plan   : fp.linear(W, keep), its backward the plan's transposed call;
  dense  : adapters.drop_feature(x, p, K) and the batched x_views @ W with autograd -- the masked copies are part of every step;
  csr    : torch.sparse CSR, x_csr @ (keep[k][:, None] * W) per view with autograd.
Medians of 5 after a warm-up of every shape, host clock around a synchronise; the five times are printed too.  Per shape and Fout
also: the plan's build time (count + build, median of 3), the steps after which the plan has paid for its build against either
torch side (build / (torch - plan), forward + backward), every side's peak memory over its forward + backward, and whether two
runs returned equal bits on each side.  Prints one JSON line per shape and Fout (and appends it to --out).  Needs an MI355X; reads
nothing outside the repository.

    python tools/feature_latency.py
    python tools/feature_latency.py --shapes cora --no-torch        # the calls alone (for rocprofv3 --kernel-trace --stats)
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

from rlap_amd import adapters, ops  # noqa: E402

SHAPES = {"cora": (2708, 1433, 18), "cs": (18333, 6805, None), "physics": (34493, 8415, None)}
K, P = 2, 0.3


def features(n, fin, nz, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    cols = torch.randint(fin, (n, nz), generator=gen, device="cuda")
    x = torch.zeros((n, fin), dtype=torch.float32, device="cuda").scatter_(1, cols, 1.0)
    return x / x.sum(1, keepdim=True)


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, res


def alternate(sides, reps):
    """{name: (median ms, the times, whether every run gave the warm-up's bits)}: the sides take turns, rep by rep."""
    first = {}
    for name, fn in sides.items():
        first[name] = fn()
        torch.cuda.synchronize()
    ts, same = {name: [] for name in sides}, {name: True for name in sides}
    for _ in range(reps):
        for name, fn in sides.items():
            t, res = once(fn)
            ts[name].append(t)
            same[name] = same[name] and all(bool(torch.equal(a, b)) for a, b in zip(res, first[name]))
            del res
    return {name: (statistics.median(ts[name]), [round(t, 4) for t in ts[name]], same[name]) for name in sides}


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = fn()
    torch.cuda.synchronize()
    del res
    return int(torch.cuda.max_memory_allocated() - base)


def run(name, n, fin, nz, fout, args, fh, quiet=False):
    x = features(n, fin, nz, n + fin)
    gen = torch.Generator(device="cuda").manual_seed(fout)
    w = (torch.rand((fin, fout), generator=gen, device="cuda") - 0.5) / 8
    gy = torch.randn((K, n, fout), generator=gen, device="cuda")
    mgen = torch.Generator(device="cuda").manual_seed(5)
    keep = ops.feature_masks(fin, P, K, generator=mgen)
    builds = [once(lambda: ops.feature_plan(x))[0] for _ in range(3)]
    fp = ops.feature_plan(x)
    rec = {"shape": name, "N": n, "Fin": fin, "nz_per_row": nz, "nnz": fp.nnz, "Fout": fout, "K": K, "p": P, "plan_bytes": fp.nbytes,
           "build_ms": round(statistics.median(builds), 4), "build_runs_ms": [round(t, 4) for t in builds],
           "longest_forward": fp.info["longest_forward"], "longest_transposed": fp.info["longest_transposed"],
           "chunks_transposed": fp.info["chunks_transposed"]}

    def plan_forward():
        return [fp.linear(w, keep)]

    def plan_both():
        tw = w.detach().clone().requires_grad_(True)
        fp.linear(tw, keep).backward(gy)
        return [tw.grad]

    def dense_views(tw):
        g = torch.Generator(device="cuda").manual_seed(5)
        return adapters.drop_feature(x, P, K, generator=g) @ tw

    def dense_forward():
        with torch.no_grad():
            return [dense_views(w)]

    def dense_both():
        tw = w.detach().clone().requires_grad_(True)
        dense_views(tw).backward(gy)
        return [tw.grad]

    fwd, both = {"plan": plan_forward}, {"plan": plan_both}
    if not args.no_torch:
        fwd["dense"], both["dense"] = dense_forward, dense_both
        try:
            x_csr = x.to_sparse_csr()
            kf = keep.to(torch.float32)

            def csr_views(tw):
                return torch.stack([x_csr @ (kf[k][:, None] * tw) for k in range(K)])

            def csr_forward():
                with torch.no_grad():
                    return [csr_views(w)]

            def csr_both():
                tw = w.detach().clone().requires_grad_(True)
                csr_views(tw).backward(gy)
                return [tw.grad]

            csr_both()
            torch.cuda.synchronize()
            fwd["csr"], both["csr"] = csr_forward, csr_both
        except Exception as e:   # (a torch build without the sparse product or its gradient: said, not hidden)
            rec["csr_error"] = f"{type(e).__name__}: {e}"[:200]
    f, b = alternate(fwd, args.reps), alternate(both, args.reps)
    for side in fwd:
        rec.update({f"{side}_forward_ms": round(f[side][0], 4), f"{side}_forward_runs_ms": f[side][1], f"{side}_forward_repeats_bit_for_bit": f[side][2],
                    f"{side}_forward_backward_ms": round(b[side][0], 4), f"{side}_forward_backward_runs_ms": b[side][1],
                    f"{side}_gradients_repeat_bit_for_bit": b[side][2], f"{side}_peak_bytes": peak_of(both[side])})
        if side != "plan":
            rec[f"{side}_forward_over_plan"] = round(f[side][0] / f["plan"][0], 3)
            rec[f"{side}_forward_backward_over_plan"] = round(b[side][0] / b["plan"][0], 3)
            gain = b[side][0] - b["plan"][0]
            rec[f"steps_to_pay_build_vs_{side}"] = round(rec["build_ms"] / gain, 2) if gain > 0 else None
    if not args.no_torch:   # the two formulations compute the same product: the worst difference, relative to the largest value
        yp, yd = plan_forward()[0], dense_forward()[0]
        rec["max_abs_diff_plan_dense"] = float((yp - yd).abs().max())
        rec["max_abs_value"] = float(yd.abs().max())
    line = json.dumps(rec)
    if not quiet:
        print(line, flush=True)
    if fh is not None:
        fh.write(line + "\n")
        fh.flush()
    del x, w, gy, fp
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--fouts", default="256,512")
    ap.add_argument("--nz", type=int, default=32, help="non-zeros a row of the shapes whose real density is not known")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="time the calls alone")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    fh = open(args.out, "a") if args.out else None
    cases = [(name, SHAPES[name][0], SHAPES[name][1], SHAPES[name][2] or args.nz, int(fo)) for name in args.shapes.split(",") for fo in args.fouts.split(",")]
    warm = argparse.Namespace(**{**vars(args), "reps": 1})
    for name, n, fin, nz, fo in cases:   # a warm-up of every shape before anything is timed
        run(name, n, fin, nz, fo, warm, None, quiet=True)
    for name, n, fin, nz, fo in cases:
        run(name, n, fin, nz, fo, args, fh)


if __name__ == "__main__":
    main()
