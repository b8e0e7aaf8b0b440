"""tests/spectra.py: every closed-form largest eigenvalue against numpy's dense eigvalsh at small sizes, and every builder's rows in
the layout the output pass writes (symmetric, no duplicates, grouped by column).  No GPU."""
import numpy as np
import pytest

import spectra

BUILDERS = {
    "star_1": lambda: spectra.star(1),
    "star_7": lambda: spectra.star(7),
    "star_299": lambda: spectra.star(299),
    "bipartite_1_1": lambda: spectra.complete_bipartite(1, 1),
    "bipartite_3_5": lambda: spectra.complete_bipartite(3, 5),
    "bipartite_17_40": lambda: spectra.complete_bipartite(17, 40),
    "wheel_4": lambda: spectra.wheel(4),
    "wheel_5": lambda: spectra.wheel(5),
    "wheel_101": lambda: spectra.wheel(101),
    "cycle_3": lambda: spectra.cycle(3),
    "cycle_4": lambda: spectra.cycle(4),
    "cycle_257": lambda: spectra.cycle(257),
    "hypercube_1": lambda: spectra.hypercube(1),
    "hypercube_3": lambda: spectra.hypercube(3),
    "hypercube_8": lambda: spectra.hypercube(8),
    "torus_3_3": lambda: spectra.torus(3, 3),
    "torus_4_7": lambda: spectra.torus(4, 7),
    "torus_12_25": lambda: spectra.torus(12, 25),
    "tree_2_1": lambda: spectra.kary_tree(2, 1),
    "tree_2_7": lambda: spectra.kary_tree(2, 7),
    "tree_3_4": lambda: spectra.kary_tree(3, 4),
    "tree_5_3": lambda: spectra.kary_tree(5, 3),
    "grid_1_2": lambda: spectra.grid(1, 2),
    "grid_2_2": lambda: spectra.grid(2, 2),
    "grid_7_9": lambda: spectra.grid(7, 9),
    "grid_10_30": lambda: spectra.grid(10, 30),
    "path_2": lambda: spectra.path(2),
    "path_3": lambda: spectra.path(3),
    "path_300": lambda: spectra.path(300),
    "union_grid_star": lambda: spectra.union(spectra.grid(12, 12), spectra.star(16)),
    "union_star_cycle_path": lambda: spectra.union(spectra.star(5), spectra.cycle(40), spectra.path(9)),
    "scaled_grid": lambda: spectra.scaled(spectra.grid(9, 11), 0.375),
    "scaled_tree": lambda: spectra.scaled(spectra.kary_tree(3, 3), 2.0 ** 20),
    "scaled_wheel": lambda: spectra.scaled(spectra.wheel(30), 1e-3),
}


def check_layout(g):
    sc = g.sc
    assert sc.dtype == np.float64 and sc.ndim == 2 and sc.shape[1] == 3
    r, c, w = sc[:, 0], sc[:, 1], sc[:, 2]
    assert np.all(r == np.floor(r)) and np.all(c == np.floor(c))
    ri, ci = r.astype(np.int64), c.astype(np.int64)
    assert ri.min() >= 0 and ci.min() >= 0 and max(ri.max(), ci.max()) < g.n
    assert not np.any(ri == ci), "self loop"
    # grouped by column: sorted by (col, row), which also makes every pair appear once
    key = ci * g.n + ri
    assert np.all(np.diff(key) > 0), "rows not sorted by (col, row), or a duplicate"
    # every id has a column (no isolated node: the node count is n)
    assert np.array_equal(np.unique(ci), np.arange(g.n))
    # symmetric, weights included
    fwd = {(a, b): x for a, b, x in zip(ri.tolist(), ci.tolist(), w.tolist())}
    for (a, b), x in fwd.items():
        assert fwd.get((b, a)) == x, (a, b)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_closed_form_against_eigvalsh(name):
    g = BUILDERS[name]()
    assert g.n <= 300
    check_layout(g)
    A = spectra.dense(g)
    assert np.array_equal(A, A.T)
    ref = np.linalg.eigvalsh(A)[-1]
    assert abs(g.lam - ref) <= 1e-12 * abs(ref), (name, g.lam, ref)


def test_node_counts():
    assert spectra.star(9).n == 10
    assert spectra.complete_bipartite(4, 6).n == 10
    assert spectra.hypercube(5).n == 32
    assert spectra.torus(5, 6).n == 30
    assert spectra.kary_tree(2, 12).n == 8191
    assert spectra.kary_tree(3, 4).n == (3 ** 5 - 1) // 2
    assert spectra.grid(60, 140).n == 8400
    assert spectra.union(spectra.star(3), spectra.path(5)).n == 9
    # rows: twice the undirected edges
    assert spectra.hypercube(13).sc.shape[0] == 13 * 8192
    assert spectra.grid(85, 85).sc.shape[0] == 2 * 2 * 85 * 84
    assert spectra.complete_bipartite(2, 7165).sc.shape[0] == 2 * 2 * 7165


@pytest.mark.parametrize("big", ["star", "cycle", "hypercube", "torus", "tree", "grid", "path", "bipartite"])
def test_layout_at_test_sizes(big):
    """The sizes the GPU tests run, checked for layout (their lambdas are too large for a dense reference here)."""
    g = {"star": lambda: spectra.star(7169), "cycle": lambda: spectra.cycle(8000), "hypercube": lambda: spectra.hypercube(13),
         "torus": lambda: spectra.torus(90, 91), "tree": lambda: spectra.kary_tree(2, 12), "grid": lambda: spectra.grid(60, 140),
         "path": lambda: spectra.path(9000), "bipartite": lambda: spectra.complete_bipartite(3, 7166)}[big]()
    sc = g.sc
    ri, ci = sc[:, 0].astype(np.int64), sc[:, 1].astype(np.int64)
    key = ci * g.n + ri
    assert np.all(np.diff(key) > 0)
    assert np.array_equal(np.unique(ci), np.arange(g.n))
    rev = np.sort(ri * g.n + ci)
    assert np.array_equal(rev, key)


def test_pack_without_and_with_node_ptr():
    gs = [spectra.star(3), None, spectra.path(5), spectra.cycle(4)]
    sc, ptr = spectra.pack(gs)
    assert ptr.tolist() == [0, 6, 6, 14, 22]
    assert np.array_equal(sc[6:14], spectra.path(5).sc)
    # node_ptr: G = 2 graphs of 5 and 4 ids; segment s is graph s % 2
    sc, ptr = spectra.pack(gs, node_ptr=[0, 5, 9])
    assert ptr.tolist() == [0, 6, 6, 14, 22]
    assert np.array_equal(sc[0:6, :2], spectra.star(3).sc[:, :2])
    assert np.array_equal(sc[6:14, :2], spectra.path(5).sc[:, :2])          # segment 2: graph 0, offset 0
    assert np.array_equal(sc[14:22, :2], spectra.cycle(4).sc[:, :2] + 5)    # segment 3: graph 1, offset 5
    with pytest.raises(AssertionError):
        spectra.pack([spectra.path(5), spectra.path(6)], node_ptr=[0, 5, 10])   # path(6) does not fit graph 1's 5 ids
    sc, ptr = spectra.pack([None, None])
    assert sc.shape == (0, 3) and ptr.tolist() == [0, 0, 0]
