"""The graphs, parameters and seeds of the node-sampling tests (rlap_node_sample, ops.sample_subgraphs), shared by
tests/test_node_sample_cpu.py and the tests/test_gpu_node_sample*.py files: the CPU suite ties the host mirror to numpy and pure
Python on exactly these inputs, the GPU suite compares the device with the mirror bit for bit."""
import numpy as np

from edge_drop_cases import MAX_GRID_ROWS, STRIDE_E, STRIDE_N, stride_rows  # noqa: F401  (one constant, one large input for the three calls)
from util import ba_graph

ROW_TILE = 2048                     # rows a workgroup flips (rlap_nodesample.h::ROW_TILE; the CPU suite asserts the equality)
SEED = 20
PS = (0.3, 0.45)
HUB = 513                           # outgoing rows of the hub
TILE_EDGE_ROWS = (0, 1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 3 * ROW_TILE + 5)
WORD_EDGE_NODES = (1, 63, 64, 65, 129, 4097)
WALKER_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257)
WALK_LENGTHS = (0, 1, 10)


TOP_ID_NODES = (4097, 65537)        # the top id in a bitmap word of its own: bit 0 of word 64, of word 1,024
TOP_ID_WALKERS = 4                  # walkers a node: enough that the mirror's walks start on the top id, leave it and arrive at it


def top_id_rows(n):
    """random_rows(300, n) with the top id written in as a source (rows 0..2) and as a target (rows 1..4): two loop rows on it, one
    row that leaves it and two that arrive from other nodes."""
    src, dst, _ = random_rows(300, n)
    src[:3] = n - 1
    dst[1:5] = n - 1
    return src, dst, n


def top_id_walk(n):
    return dict(scheme="walk", num_seeds=[TOP_ID_WALKERS * n, 3], walk_length=2, seed=1)


def passes_through(walks, v):
    """(a walk starts on v, a walk arrives at v from another node, a walk leaves v for another node)."""
    at = walks == v
    return bool(at[:, 0].any()), bool((~at[:, :-1] & at[:, 1:]).any()), bool((at[:, :-1] & ~at[:, 1:]).any())


def directed():
    """A hand-made directed list: duplicates, loop rows (3 -> 3, 5 -> 5, 4 -> 4), a sink (9: rows in, none out), id 7 without rows,
    and a hub (6) with HUB outgoing rows to ids of their own, the hub's rows in the middle of the list."""
    src = [0, 1, 1, 2, 3, 3, 3, 4, 5, 5, 6]
    dst = [1, 2, 2, 0, 3, 4, 4, 5, 5, 6, 9]
    src += [6] * HUB
    dst += list(range(10, 10 + HUB))
    src += [2, 0, 8, 8, 4, 10, 11]
    dst += [3, 1, 0, 1, 4, 6, 6]
    return np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), 10 + HUB


def ba300():
    ei = ba_graph(300, 3, 7)
    return ei[0].copy(), ei[1].copy(), 300


def two_ba50():
    """The disjoint union of two BA(50, 2): a batch as the reference hands it to an augmentor."""
    g0, g1 = ba_graph(50, 2, 1), ba_graph(50, 2, 2)
    return np.concatenate([g0[0], g1[0] + 50]), np.concatenate([g0[1], g1[1] + 50]), 100


def star7():
    """Centre 0 with 7 outgoing rows to 1..7, nothing else: a walker on the centre picks a neighbour uniformly, then stays."""
    return np.zeros(7, dtype=np.int64), np.arange(1, 8, dtype=np.int64), 8


GRAPHS = {"directed": directed, "ba300": ba300, "two_ba50": two_ba50, "star7": star7}


def graph(name):
    src, dst, n = GRAPHS[name]()
    return np.ascontiguousarray(src), np.ascontiguousarray(dst), n


def weights(E, seed=5):
    return np.random.RandomState(seed).rand(E) + 0.5


def random_rows(E, n=97, seed=11):
    """E directed rows on n nodes for the compaction and bitmap tests."""
    rs = np.random.RandomState(seed + E + 7 * n)
    return rs.randint(0, n, E).astype(np.int64), rs.randint(0, n, E).astype(np.int64), n
