"""The graphs, parameters and seeds of the edge-adding tests (rlap_edge_add, ops.add_edges), shared by
tests/test_edge_add_cpu.py and the tests/test_gpu_edge_add*.py files: the CPU suite ties the host mirror to numpy and pure Python on
these inputs, the GPU suite compares the device with the mirror bit for bit."""
import numpy as np

from edge_drop_cases import MAX_GRID_ROWS, STRIDE_E, STRIDE_N, stride_rows  # noqa: F401  (one constant, one large input for the three calls)
from util import ba_graph

M64 = (1 << 64) - 1
WRAP_SEEDS = range(400)
WRAP_RATIOS = (1.5, 0.5)
ROW_TILE = 2048                     # merged positions a workgroup owns (rlap_edgeadd.h::ROW_TILE; the CPU suite asserts the equality)
T = ROW_TILE
SEED = 20
RATIOS = (0.3, 0.4)
# (n_a, num_add), each in {0, 1, T - 1, T, T + 1, 2 T + 1}, whose merged length n_a + n_b lies on both sides of a multiple of the tile: n_b <= num_add is what the draws leave
# distinct, so equal counts are paired with the ones just around them
TILE_EDGE_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1), (0, T - 1), (0, T), (0, T + 1), (0, 2 * T + 1), (T - 1, 0), (T, 0), (T + 1, 0), (2 * T + 1, 0),
                   (T - 1, 1), (1, T - 1), (T, 1), (1, T), (T - 1, T + 1), (T + 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, 1), (1, 2 * T + 1),
                   (2 * T + 1, 2 * T + 1), (T - 1, 2 * T + 1)]
WIDE_N = 4097 * 4099                # ids wide enough that random pairs are distinct: n_a and n_b are what is asked for


def ba300():
    ei = ba_graph(300, 3, 7)
    return ei[0].copy(), ei[1].copy(), 300


def two_ba50():
    """The disjoint union of two BA(50, 2): a batch as the reference hands it to an augmentor."""
    g0, g1 = ba_graph(50, 2, 1), ba_graph(50, 2, 2)
    return np.concatenate([g0[0], g1[0] + 50]), np.concatenate([g0[1], g1[1] + 50]), 100


def messy():
    """Directed rows with duplicates and loops on 40 nodes, in no order."""
    rs = np.random.RandomState(3)
    return rs.randint(0, 40, 700).astype(np.int64), rs.randint(0, 40, 700).astype(np.int64), 40


GRAPHS = {"ba300": ba300, "two_ba50": two_ba50, "messy": messy}


def graph(name):
    src, dst, n = GRAPHS[name]()
    return np.ascontiguousarray(src), np.ascontiguousarray(dst), n


def weights(E, seed=5):
    """General float64 weights: sums depend on their order."""
    return np.random.RandomState(seed).rand(E) * 3.0 + 0.1


def dyadic(E, seed=6):
    """Multiples of 1/8 below 4: every sum of fewer than 2^48 of them is exact in any order."""
    return np.random.RandomState(seed).randint(1, 32, E).astype(np.float64) / 8.0


def distinct_rows(n_a, n=WIDE_N, seed=11, low=0, high=None):
    """n_a distinct (source, target) pairs with ids in [low, high), in no order."""
    high = n if high is None else high
    rs = np.random.RandomState(seed + n_a)
    span = high - low
    key = np.unique(rs.randint(0, span * span, 2 * n_a + 8, dtype=np.int64))
    key = rs.permutation(key)[:n_a]
    assert key.size == n_a
    return (key // span + low).astype(np.int64), (key % span + low).astype(np.int64), n


def tiny_unsorted(seed):
    """2 to 12 rows on 3 to 6 nodes: a key set of 4 to 24 slots, small enough that a probe often reaches the table's end."""
    r = np.random.RandomState(seed)
    E = r.randint(2, 13)
    N = r.randint(3, 7)
    return r.randint(0, N, E).astype(np.int64), r.randint(0, N, E).astype(np.int64), int(N)


# ---- a model of the key set of an input whose keys do not ascend (rlap_edgeadd.hip: 2 E slots, home = mix64(key) % slots, linear
# probing that wraps at the table's end).  It is used only to choose inputs: what the call returns is compared with the mirror,
# which finds the same counts by sorting.
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def id_bits(n):
    b = 1
    while b < 31 and (1 << b) < n:
        b += 1
    return b


def pair_keys(src, dst, n):
    b = id_bits(n)
    return [(int(s) << b) | int(t) for s, t in zip(src, dst)]


def table_of(keys):
    """The table after a sequential insertion of `keys`, and whether a key went into a slot below its home: the occupied run then
    crosses the table's end.  The set of occupied slots does not depend on the order of insertion."""
    slots = 2 * len(keys)
    table, wrapped = [None] * slots, False
    for key in keys:
        home = h = mix64(key) % slots
        while table[h] is not None and table[h] != key:
            h = 0 if h + 1 == slots else h + 1
        wrapped = wrapped or h < home
        table[h] = key
    return table, wrapped


def probe(table, key):
    """(found, crossed): a probe for `key` as the device makes it, and whether it stepped from the last slot to slot 0."""
    slots = len(table)
    h, crossed = mix64(key) % slots, False
    for _ in range(slots):
        if table[h] == key:
            return True, crossed
        if table[h] is None:
            return False, crossed
        crossed = crossed or h + 1 == slots
        h = 0 if h + 1 == slots else h + 1
    return False, crossed


def wrapping_inputs():
    """The seeds of WRAP_SEEDS whose tiny_unsorted input has keys that do not ascend and a table whose occupied run crosses its end."""
    out = []
    for seed in WRAP_SEEDS:
        src, dst, n = tiny_unsorted(seed)
        keys = pair_keys(src, dst, n)
        if any(a > b for a, b in zip(keys, keys[1:])) and table_of(keys)[1]:
            out.append(seed)
    return out


def coalesced(src, dst, n):
    """The rows sorted by (source, target), duplicates removed: what a coalesced PyG graph is."""
    key = np.unique(src * n + dst)
    return key // n, key % n


def python_reference(src, dst, w, added, n):
    """One coalesced view by the prose of the contract, in Python: the pairs ascending; a pair's weight is the sum of its input
    rows, added up in input order from 0.0, plus -- in one addition -- the number of its added rows."""
    s_in, c_add = {}, {}
    for e in range(len(src)):
        pair = (int(src[e]), int(dst[e]))
        s_in[pair] = s_in.get(pair, 0.0) + (1.0 if w is None else float(w[e]))
    for s, t in added.tolist():
        c_add[(s, t)] = c_add.get((s, t), 0) + 1
    pairs = sorted(set(s_in) | set(c_add))
    return np.array([[s, t, s_in.get((s, t), 0.0) + float(c_add.get((s, t), 0))] for s, t in pairs], dtype=np.float64).reshape(-1, 3)
