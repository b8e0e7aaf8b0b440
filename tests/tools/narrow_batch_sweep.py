"""Candidates per round of the degree order's 16-slot kernel (RLAP_NARROW_BATCH) against elimination time on BA(1M,10), degree/asc:
usage: narrow_batch_sweep.py off 256 224 192 160 ...   ("off" = RLAP_NARROW=0, the 32-slot kernel alone)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from rlap_amd import graphs, ops
n, m = 1000000, 10
ei = graphs.barabasi_albert(n, m, 2).cuda()
ops.set_timing(True)
ref = None
for nb in sys.argv[1:]:
    if nb == "off":
        os.environ["RLAP_NARROW"] = "0"
    else:
        os.environ.pop("RLAP_NARROW", None)
        os.environ["RLAP_NARROW_BATCH"] = nb
    ts = []
    for r in range(4):
        out = ops.approximate_cholesky(ei, None, n, n // 2, "degree", "asc", return_device="same")
        st = dict(ops.last_stats)
        if r:
            ts.append(st["ms_elim"])
    if ref is None:
        ref = out
    print(f"narrow_batch {nb}: ms_elim {min(ts):.2f} .. {max(ts):.2f}  rounds {st['n_rounds']} narrow {st['n_rounds_narrow']} "
          f"singles {st['n_singles']} same_rows {bool(torch.equal(out, ref))}", flush=True)
