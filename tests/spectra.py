"""Graphs whose largest adjacency eigenvalue is known in closed form, at any size (numpy only).

Every builder returns a Graph: `sc`, the graph's (m, 3) float64 rows [row, col, w] grouped by column (sorted by (col, row)), the
layout the output pass writes; `n`, its node count (ids 0..n-1, every id with a column of its own); and `lam`, the exact largest
eigenvalue of its symmetric adjacency matrix (unit weights unless scaled), evaluated in float64.  They are independent references
for the snapshot statistics' Lanczos: Lanczos from the all-ones vector converges on them in very different numbers of steps
(regular graphs break down at step 1, stars and complete bipartite graphs at step 2, paths need about n / 2)."""
from collections import namedtuple

import numpy as np

Graph = namedtuple("Graph", "sc n lam")


def from_edges(a, b, n, lam, w=1.0):
    """Graph of the undirected edges (a[i], b[i]) on ids [0, n): both directions, duplicates merged, rows sorted by (col, row)."""
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    assert not np.any(a == b), "no self loops"
    r = np.concatenate([a, b])
    c = np.concatenate([b, a])
    key = np.unique(c * n + r)
    sc = np.empty((key.size, 3), dtype=np.float64)
    sc[:, 0] = key % n
    sc[:, 1] = key // n
    sc[:, 2] = w
    return Graph(sc, int(n), float(lam))


def star(k):
    """K_{1,k}: hub 0, leaves 1..k; sqrt(k)."""
    leaves = np.arange(1, k + 1)
    return from_edges(np.zeros(k, dtype=np.int64), leaves, k + 1, np.sqrt(k))


def complete_bipartite(a, b):
    """K_{a,b}: ids [0, a) against [a, a + b); sqrt(a b)."""
    x, y = np.meshgrid(np.arange(a), np.arange(a, a + b), indexing="ij")
    return from_edges(x.ravel(), y.ravel(), a + b, np.sqrt(float(a) * float(b)))


def wheel(n):
    """Hub 0 joined to a cycle 1..n-1 (n >= 4); 1 + sqrt(n)."""
    assert n >= 4
    rim = np.arange(1, n)
    a = np.concatenate([np.zeros(n - 1, dtype=np.int64), rim])
    b = np.concatenate([rim, np.roll(rim, -1)])
    return from_edges(a, b, n, 1.0 + np.sqrt(n))


def cycle(n):
    """C_n (n >= 3); 2."""
    assert n >= 3
    i = np.arange(n)
    return from_edges(i, (i + 1) % n, n, 2.0)


def path(n):
    """P_n (n >= 2); 2 cos(pi / (n + 1))."""
    i = np.arange(n - 1)
    return from_edges(i, i + 1, n, 2.0 * np.cos(np.pi / (n + 1)))


def hypercube(d):
    """Q_d: ids 0..2^d - 1, joined when they differ in one bit; d."""
    i = np.arange(1 << d)
    a = np.concatenate([i for _ in range(d)])
    b = np.concatenate([i ^ (1 << k) for k in range(d)])
    return from_edges(a, b, 1 << d, float(d))


def _product_edges(ea, na, eb, nb):
    """Edges of the Cartesian product G x H (id = i * nb + j) from the edge lists of G (na nodes) and H (nb nodes)."""
    i = np.arange(na)
    j = np.arange(nb)
    a1 = (i[:, None] * nb + eb[0][None, :]).ravel()
    b1 = (i[:, None] * nb + eb[1][None, :]).ravel()
    a2 = (ea[0][:, None] * nb + j[None, :]).ravel()
    b2 = (ea[1][:, None] * nb + j[None, :]).ravel()
    return np.concatenate([a1, a2]), np.concatenate([b1, b2])


def _path_edges(n):
    i = np.arange(n - 1)
    return i, i + 1


def _cycle_edges(n):
    i = np.arange(n)
    return i, (i + 1) % n


def grid(a, b):
    """P_a x P_b; 2 cos(pi / (a + 1)) + 2 cos(pi / (b + 1))."""
    x, y = _product_edges(_path_edges(a), a, _path_edges(b), b)
    return from_edges(x, y, a * b, 2.0 * np.cos(np.pi / (a + 1)) + 2.0 * np.cos(np.pi / (b + 1)))


def torus(a, b):
    """C_a x C_b (a, b >= 3); 4."""
    assert a >= 3 and b >= 3
    x, y = _product_edges(_cycle_edges(a), a, _cycle_edges(b), b)
    return from_edges(x, y, a * b, 4.0)


def kary_tree(k, h):
    """Balanced k-ary tree of depth h (root 0, node i's children k i + 1 .. k i + k; (k^(h+1) - 1) / (k - 1) nodes, k >= 2);
    2 sqrt(k) cos(pi / (h + 2)): its levels reduce it to a path of h + 1 nodes with couplings sqrt(k)."""
    assert k >= 2 and h >= 1
    n = (k ** (h + 1) - 1) // (k - 1)
    child = np.arange(1, n)
    return from_edges((child - 1) // k, child, n, 2.0 * np.sqrt(k) * np.cos(np.pi / (h + 2)))


def union(*graphs):
    """Disjoint union: graph i's ids shifted past those before it; the largest lambda over the parts."""
    off = 0
    parts = []
    for g in graphs:
        s = g.sc.copy()
        s[:, :2] += off
        parts.append(s)
        off += g.n
    return Graph(np.concatenate(parts), off, max(g.lam for g in graphs))


def scaled(g, c):
    """Every weight c (c > 0): c lambda."""
    s = g.sc.copy()
    s[:, 2] = c
    return Graph(s, g.n, c * g.lam)


def dense(g):
    """The graph's (n, n) float64 adjacency matrix (weights summed over duplicate rows)."""
    A = np.zeros((g.n, g.n))
    np.add.at(A, (g.sc[:, 0].astype(np.int64), g.sc[:, 1].astype(np.int64)), g.sc[:, 2])
    return A


def pack(graphs, node_ptr=None):
    """Segments `graphs` (None: an empty segment) as one call's (sc, ptr): numpy (m, 3) rows and S + 1 int64 offsets.  With
    `node_ptr` (G + 1 offsets, G dividing S) segment s is graph s % G: its ids are shifted to start at node_ptr[s % G] and must fit
    below node_ptr[s % G + 1]."""
    if node_ptr is not None:
        node_ptr = np.asarray(node_ptr, dtype=np.int64)
        G = node_ptr.size - 1
        assert len(graphs) % G == 0
    parts, ptr = [], [0]
    for s, g in enumerate(graphs):
        if g is None:
            ptr.append(ptr[-1])
            continue
        x = g.sc.copy()
        if node_ptr is not None:
            lo, hi = int(node_ptr[s % G]), int(node_ptr[s % G + 1])
            assert g.n <= hi - lo, (s, g.n, lo, hi)
            x[:, :2] += lo
        parts.append(x)
        ptr.append(ptr[-1] + x.shape[0])
    sc = np.concatenate(parts) if parts else np.zeros((0, 3))
    return sc, np.asarray(ptr, dtype=np.int64)
