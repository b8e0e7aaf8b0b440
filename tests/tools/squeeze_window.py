"""The window the squeeze passes are for, on BA(1M,10) (the bench's graph), degree/asc: the 16-slot kernel's first hand-over (largest
num_remove whose rounds are all narrow and without single vertices, by bisection) and the elimination time to that point, to
pop 385,000 (just in front of the last hand-over with the passes on) and to 500,000 (the bench's call).
usage: python tests/tools/squeeze_window.py TREE OUTFILE   (TREE: checkout whose build is measured, e.g. `.`)"""
import os
import statistics
import sys

tree = os.path.abspath(sys.argv[1])
out = sys.argv[2]
sys.path.insert(0, tree)
import torch  # noqa: E402
from rlap_amd import graphs, ops  # noqa: E402

ops.set_timing(True)
n = 1_000_000
ei = graphs.barabasi_albert(n, 10, 2).cuda()


def run(t, reps=0):
    ops.approximate_cholesky(ei, None, n, t, "degree", "asc", seed=7, return_device="same")
    st = dict(ops.last_stats)
    if reps == 0:
        return st
    ms = []
    for _ in range(2):
        ops.approximate_cholesky(ei, None, n, t, "degree", "asc", seed=7, return_device="same")
    for _ in range(reps):
        ops.approximate_cholesky(ei, None, n, t, "degree", "asc", seed=7, return_device="same")
        torch.cuda.synchronize()
        ms.append(ops.last_stats["ms_elim"])
    return st, statistics.median(ms), min(ms), max(ms)


lines = [f"# python tests/tools/squeeze_window.py (tree {os.path.basename(tree)}): BA(1M,10) seed 2, degree/asc, seed 7; ms_elim median of 5 after 2 warm-ups"]
lo, hi = 1, 500_000   # largest t with n_rounds_narrow == n_rounds
assert run(lo)["n_rounds_narrow"] == run(lo)["n_rounds"]
while lo < hi:
    mid = (lo + hi + 1) // 2
    st = run(mid)
    if st["n_rounds_narrow"] == st["n_rounds"] and st["n_singles"] == 0:
        lo = mid
    else:
        hi = mid - 1
lines.append(f"hand-over: largest t with n_rounds_narrow == n_rounds: {lo}")
for t in (lo, 385_000, 500_000):
    st, med, mn, mx = run(t, 5)
    lines.append(f"t={t}: ms_elim median {med:.2f} (min {mn:.2f} max {mx:.2f}) n_rounds {st['n_rounds']} n_rounds_narrow {st['n_rounds_narrow']} "
                 f"n_singles {st['n_singles']} n_squeezes {st.get('n_squeezes', '-')}")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
