"""What the round kernels' skip rule (rlap_core.h::cand_touches) removes on a graph of the bench's size: the CPU mirror with the rule
(tests/csrc/host_mirror_skip.cc; no move cap, no record cap) on tests/util.ba_graph(1_000_000, 10, 2), seed 7, degree/asc, t = n/2 --
touched pairs over all pairs, contended records with and without the rule, rounds.  A tool, not a test: the graph takes minutes to
generate.  usage (from the repository root): python tests/tools/skip_stats.py [candidates per 16-slot round [per 32-slot round]]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from util import ba_graph
from test_skip_mirror import load_skip_mirror, skip_call
B = int(sys.argv[1]) if len(sys.argv) > 1 else 192
B32 = int(sys.argv[2]) if len(sys.argv) > 2 else 128
n = 1_000_000
t0 = time.time()
ei = ba_graph(n, 10, 2)
print(f"BA({n},10): {ei.shape[1]} entries ({time.time() - t0:.0f} s)", flush=True)
lib = load_skip_mirror()
for bc in (16, 32):
    t0 = time.time()
    _, _, st = skip_call(lib, ei, None, n, n // 2, "asc", bc, seed=7, B=B, B32=B32)
    print(f"records of {bc} slots first, {B if bc == 16 else B32} candidates per round ({time.time() - t0:.0f} s): {st}")
    print(f"   touched pairs {st['pairs_touched']} of {st['pairs']} ({st['pairs_touched'] / st['pairs']:.3f}); contended records "
          f"{st['contended_touched']} with the rule, {st['contended_all']} without ({st['contended_touched'] / max(st['contended_all'], 1):.3f})", flush=True)
