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
