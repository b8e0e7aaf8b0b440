"""Elimination time of the bench's call (BA(1M,10), degree/asc) against the candidates per round of the 16-slot launches behind a
squeeze pass (RLAP_NARROW_BATCH_LATE), and with the passes off.  usage (from the repository root): python tests/tools/narrow_batch_late_sweep.py"""
import os, statistics, sys
sys.path.insert(0, os.getcwd())
import torch
from rlap_amd import graphs, ops
ops.set_timing(True)
n = 1_000_000
ei = graphs.barabasi_albert(n, 10, 2).cuda()
def med(t=n // 2):
    ms = []
    for i in range(7):
        ops.approximate_cholesky(ei, None, n, t, "degree", "asc", seed=7, return_device="same")
        torch.cuda.synchronize()
        if i >= 2: ms.append(ops.last_stats["ms_elim"])
    st = ops.last_stats
    return f"ms_elim median {statistics.median(ms):.2f} (min {min(ms):.2f} max {max(ms):.2f}) n_rounds {st['n_rounds']} narrow {st['n_rounds_narrow']} singles {st['n_singles']} squeezes {st['n_squeezes']}"
os.environ["RLAP_SQUEEZE"] = "0"
print("squeeze off:", med(), flush=True)
os.environ["RLAP_SQUEEZE"] = "1"
for nb in (192, 160, 144, 128, 112, 96, 80):
    os.environ["RLAP_NARROW_BATCH_LATE"] = str(nb)
    print(f"late batch {nb}:", med(), flush=True)
    print(f"   to 385000:", med(385000), flush=True)
