"""Elimination time of the bench's call (BA(1M,10), degree/asc, t = n/2) against the candidates per round of the 16-slot kernel in front
of the first squeeze pass (RLAP_NARROW_BATCH) and behind one (RLAP_NARROW_BATCH_LATE).
usage (from the repository root): python tests/tools/skip_batch_sweep.py"""
import os, statistics, sys
sys.path.insert(0, os.getcwd())
import torch
from rlap_amd import graphs, ops
ops.set_timing(True)
n = 1_000_000
ei = graphs.barabasi_albert(n, 10, 2).cuda()
ref = None
def med():
    global ref
    ms = []
    for i in range(6):
        out = ops.approximate_cholesky(ei, None, n, n // 2, "degree", "asc", seed=7, return_device="same")
        torch.cuda.synchronize()
        if i >= 2: ms.append(ops.last_stats["ms_elim"])
    if ref is None: ref = out
    st = ops.last_stats
    return (f"ms_elim median {statistics.median(ms):.2f} (min {min(ms):.2f} max {max(ms):.2f}) n_rounds {st['n_rounds']} narrow {st['n_rounds_narrow']} "
            f"singles {st['n_singles']} squeezes {st['n_squeezes']} retries {st['n_retries']} same_rows {bool(torch.equal(out, ref))}")
print("defaults:", med(), flush=True)
for nb in (160, 176, 192, 208, 224, 256):
    for late in (112, 128, 144, 160, 176, 192):
        os.environ["RLAP_NARROW_BATCH"] = str(nb)
        os.environ["RLAP_NARROW_BATCH_LATE"] = str(late)
        print(f"batch {nb} late {late}:", med(), flush=True)
