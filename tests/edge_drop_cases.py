"""The graphs, parameters and seeds of the edge-dropping tests (rlap_edge_drop, ops.drop_edges), shared by
tests/test_edge_drop_cpu.py and the tests/test_gpu_edge_drop*.py files: the CPU suite checks the rules on exactly these inputs and
asserts that no coin of any of them falls within BAND of its drop probability, which is what lets the GPU suite compare masks bit
for bit although the device's float64 log may differ from the host's in the last place."""
import numpy as np

from util import ba_graph

ROW_TILE = 2048                     # rows a workgroup flips (rlap_edgedrop.h::ROW_TILE; the CPU suite asserts the equality)
BAND = 1e-9                         # |u - q| below which a keep decision may depend on the last place of log
COMB_DEGREES = (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)
SCHEMES = ("uniform", "degree", "pagerank", "eigenvector")
PS, THRESHOLD, SEED = (0.3, 0.45), 0.7, 20
TILE_EDGE_ROWS = (0, 1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 3 * ROW_TILE + 5)
NODE_TILE = 256                     # nodes of a tile, and lanes of a workgroup (rlap_edgedrop.h::TILE)
MAX_GRID_ROWS = 8192 * 256          # rows one round of a strided launch covers: ED_MAX_GRID workgroups of TILE lanes (the CPU suite ties both)
# 1, 1, 2, 256 and 257 node tiles on both sides of a power of two: the stride of wg_total runs once at 65,536 nodes, twice at 65,537
NODE_EDGE_NODES = (255, 256, 257, 65536, 65537)
NODE_EDGE_ITERS = dict(pr_iters=3, evc_max_iter=5)
RUN_DEGREES = (1, 63, 64, 65, 129, 300)
MANY_PS = tuple(k / 40 for k in range(32))            # K = 32: every view a flip kernel keeps a count for
STRIDE_E, STRIDE_N, STRIDE_SEED = 2**21 + 65, 2**21 + 300, 5   # one full round of a strided launch, then one whole wave and one lane
STRIDE_ITERS = dict(pr_iters=2, evc_max_iter=3)


def _shuffled(src, dst, seed):
    order = np.random.RandomState(seed).permutation(len(src))
    return np.ascontiguousarray(src[order]), np.ascontiguousarray(dst[order])


def ba300():
    ei = ba_graph(300, 3, 7)
    return ei[0].copy(), ei[1].copy(), 300


def comb():
    """Targets 0..11 with in-degrees COMB_DEGREES from distinct sources 12, 13, ..., both directions of every edge, rows shuffled:
    every lane and accumulator edge of the list rule (16 lanes, 4 accumulators) and a list of more than 512 rows."""
    src, dst = [], []
    for j, d in enumerate(COMB_DEGREES):
        src += list(range(12, 12 + d)) + [j] * d
        dst += [j] * d + list(range(12, 12 + d))
    s, d = _shuffled(np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), 3)
    return s, d, 12 + max(COMB_DEGREES)


def directed():
    """A hand-made directed list: duplicates, loop rows, a node with rows in one direction only, id 7 without rows."""
    src = np.array([0, 1, 1, 2, 3, 3, 3, 4, 5, 5, 6, 2, 0, 8, 8, 4], dtype=np.int64)
    dst = np.array([1, 2, 2, 0, 3, 4, 4, 5, 5, 6, 0, 3, 1, 0, 1, 4], dtype=np.int64)
    return src, dst, 9


def ring64():
    a = np.arange(64, dtype=np.int64)
    b = (a + 1) % 64
    return np.concatenate([a, b]), np.concatenate([b, a]), 64


def two_ba50():
    """The disjoint union of two BA(50, 2): a batch as the reference hands it to an augmentor."""
    g0, g1 = ba_graph(50, 2, 1), ba_graph(50, 2, 2)
    return np.concatenate([g0[0], g1[0] + 50]), np.concatenate([g0[1], g1[1] + 50]), 100


def node_edge_rows(n):
    """3 n + 7 random rows on n nodes, the top id written in as a source and as a target: N at the edge of a node tile and of a
    key width."""
    E = 3 * n + 7
    rs = np.random.RandomState(11 + n)
    src, dst = rs.randint(0, n, E).astype(np.int64), rs.randint(0, n, E).astype(np.int64)
    src[:3] = n - 1
    dst[1:5] = n - 1
    return src, dst, n


def runs(front=False, by_source=False):
    """Targets 0..5 with in-degrees RUN_DEGREES, target j from its own sources j + 1, j + 2, ... (so targets 1..5 are sources too and
    no score is the same at every node), the rows in ascending target order: the runs of equal ids that a sorted row list hands to
    the wave-run counter.  `front` puts one row (0 -> 5) before them, so that every run moves one lane; `by_source` swaps the two
    ends, so that the list is sorted by source."""
    src, dst = ([0], [5]) if front else ([], [])
    for j, d in enumerate(RUN_DEGREES):
        src += list(range(j + 1, j + 1 + d))
        dst += [j] * d
    s, d = np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64)
    return (d, s, 6 + max(RUN_DEGREES)) if by_source else (s, d, 6 + max(RUN_DEGREES))


RUN_VARIANTS = {"by_target": (False, False), "by_target_front": (True, False), "by_source": (False, True), "by_source_front": (True, True)}


def run_spans(ids):
    """[first, last] positions of every run of equal neighbouring ids."""
    cut = np.flatnonzero(np.diff(ids)) + 1
    return list(zip([0] + cut.tolist(), (cut - 1).tolist() + [len(ids) - 1]))


def stride_rows():
    """More rows than one round of a strided launch covers, by one whole wave and one lane; both ends random."""
    rs = np.random.RandomState(STRIDE_SEED)
    return rs.randint(0, STRIDE_N, STRIDE_E).astype(np.int64), rs.randint(0, STRIDE_N, STRIDE_E).astype(np.int64), STRIDE_N


GRAPHS = {"ba300": ba300, "comb": comb, "directed": directed, "ring64": ring64, "two_ba50": two_ba50}
CONNECTED = ("ba300", "ring64")      # symmetric and connected: the eigenvector bound applies


def graph(name):
    src, dst, n = GRAPHS[name]()
    return np.ascontiguousarray(src), np.ascontiguousarray(dst), n


def weights(E, seed=5):
    return np.random.RandomState(seed).rand(E) + 0.5


def random_rows(E, n=97, seed=11):
    """E directed rows on n nodes for the compaction tests."""
    rs = np.random.RandomState(seed + E)
    return rs.randint(0, n, E).astype(np.int64), rs.randint(0, n, E).astype(np.int64), n


def scored_cases():
    """(graph name, scheme, aggr): every scheme on every graph by target, the three centralities by source on two of them."""
    out = [(g, s, "sink") for g in GRAPHS for s in SCHEMES]
    out += [(g, s, "source") for g in ("directed", "comb") for s in SCHEMES[1:]]
    return out
