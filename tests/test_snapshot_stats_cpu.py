"""Snapshot statistics without a GPU: the tridiagonal routines of rlap_amd/csrc/rlap_lanczos.h (compiled here with g++, the same
source the kernels of rlap_stats.hip include) against numpy, and the host-side argument checks of ops.snapshot_stats."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_lanczos.h")

WRAP = r"""
#include <vector>
#include "rlap_lanczos.h"
extern "C" {
double lz_max_eig(const double* a, const double* b, int k) { return rlap::lanczos::max_eig(a, b, k); }
int lz_count_below(const double* a, const double* b, int k, double x) {
    return rlap::lanczos::count_below(a, b, k, x, rlap::lanczos::pivmin(b, k));
}
double lz_last_component(const double* a, const double* b, int k, double theta) {
    std::vector<double> dp(k), dm(k);
    return rlap::lanczos::last_component(a, b, k, theta, dp.data(), dm.data());
}
int lz_converged(double beta, double y, double theta, double tol) { return rlap::lanczos::converged(beta, y, theta, tol) ? 1 : 0; }
}
"""


@pytest.fixture(scope="module")
def lz(tmp_path_factory):
    d = tmp_path_factory.mktemp("lanczos")
    src, so = d / "lz.cc", d / "liblz.so"
    src.write_text(WRAP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.dirname(HDR),
                           "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    dp, ci, cd = ctypes.POINTER(ctypes.c_double), ctypes.c_int, ctypes.c_double
    lib.lz_max_eig.restype = cd
    lib.lz_max_eig.argtypes = [dp, dp, ci]
    lib.lz_count_below.restype = ci
    lib.lz_count_below.argtypes = [dp, dp, ci, cd]
    lib.lz_last_component.restype = cd
    lib.lz_last_component.argtypes = [dp, dp, ci, cd]
    lib.lz_converged.restype = ci
    lib.lz_converged.argtypes = [cd, cd, cd, cd]

    class LZ:
        @staticmethod
        def _p(x):
            x = np.ascontiguousarray(x, dtype=np.float64)
            return x, x.ctypes.data_as(dp)

        def max_eig(self, a, b):
            a, pa = self._p(a)
            b, pb = self._p(b if len(b) else [0.0])
            return lib.lz_max_eig(pa, pb, len(a))

        def count_below(self, a, b, x):
            a, pa = self._p(a)
            b, pb = self._p(b if len(b) else [0.0])
            return lib.lz_count_below(pa, pb, len(a), x)

        def last_component(self, a, b, theta):
            a, pa = self._p(a)
            b, pb = self._p(b if len(b) else [0.0])
            return lib.lz_last_component(pa, pb, len(a), theta)

        def converged(self, beta, y, theta, tol):
            return bool(lib.lz_converged(beta, y, theta, tol))
    return LZ()


def tri(a, b):
    return np.diag(a) + np.diag(b, 1) + np.diag(b, -1)


def cases():
    rng = np.random.RandomState(7)
    out = [("1x1", np.array([2.5]), np.array([]))]
    for k in (2, 3, 10, 60, 200):
        out.append((f"random{k}", rng.randn(k), rng.randn(k - 1)))
    k = 40   # clustered: eigenvalues within 1e-9 of each other at the top
    out.append(("clustered", 5.0 + 1e-9 * rng.randn(k), 1e-10 * np.abs(rng.randn(k - 1))))
    out.append(("repeated", np.full(12, 3.0), np.zeros(11)))   # (T = 3 I)
    b = rng.rand(29) + 0.1
    b[[4, 17]] = 0.0
    out.append(("zero-offdiag", rng.randn(30), b))
    b = rng.rand(19) + 0.1
    b[-1] = 0.0   # the largest eigenvalue in the top block or the 1x1 block at the bottom
    a = rng.randn(20)
    out.append(("split-bottom-small", a.copy(), b.copy()))
    a[-1] = 50.0
    out.append(("split-bottom-large", a, b))
    # a Lanczos tridiagonal of a real graph (path on 50 nodes, bipartite: spectrum symmetric about 0)
    n = 50
    A = np.diag(np.ones(n - 1), 1) + np.diag(np.ones(n - 1), -1)
    al, be = lanczos_full(A, 30)
    out.append(("path-lanczos", al, be[:-1]))
    return out


def lanczos_full(A, k):
    """Lanczos with full reorthogonalisation from the normalised all-ones vector: (alpha[k], beta[k])."""
    n = A.shape[0]
    V = np.zeros((n, k + 1))
    V[:, 0] = 1.0 / np.sqrt(n)
    al, be = np.zeros(k), np.zeros(k)
    for j in range(k):
        w = A @ V[:, j]
        al[j] = w @ V[:, j]
        w -= V[:, :j + 1] @ (V[:, :j + 1].T @ w)
        w -= V[:, :j + 1] @ (V[:, :j + 1].T @ w)
        be[j] = np.linalg.norm(w)
        V[:, j + 1] = w / be[j]
    return al, be


@pytest.mark.parametrize("name,a,b", cases(), ids=[c[0] for c in cases()])
def test_bisection_matches_eigvalsh(lz, name, a, b):
    ev = np.linalg.eigvalsh(tri(a, b))
    theta = lz.max_eig(a, b)
    scale = max(1.0, np.abs(ev).max())
    assert abs(theta - ev[-1]) <= 1e-13 * scale, (theta, ev[-1])
    # Sturm counts at points between the eigenvalues
    xs = [ev[0] - 1.0, ev[-1] + 1.0] + [0.5 * (lo + hi) for lo, hi in zip(ev[:-1], ev[1:]) if hi - lo > 1e-6 * scale]
    for x in xs:
        assert lz.count_below(a, b, x) == int((ev < x).sum())


@pytest.mark.parametrize("name,a,b", cases(), ids=[c[0] for c in cases()])
def test_last_component_matches_eigenvector(lz, name, a, b):
    T = tri(a, b)
    ev, vec = np.linalg.eigh(T)
    theta = lz.max_eig(a, b)
    y = lz.last_component(a, b, theta)
    assert 0.0 <= y <= 1.0
    gap = ev[-1] - ev[-2] if len(ev) > 1 else np.inf
    if gap > 1e-6 * max(1.0, abs(ev[-1])):   # (the eigenvector is determined up to sign)
        assert abs(y - abs(vec[-1, -1])) <= 1e-8, (y, vec[-1, -1])
    else:   # a repeated top eigenvalue: some unit vector of its eigenspace has this last component
        V = vec[:, np.abs(ev - ev[-1]) <= 1e-6 * max(1.0, abs(ev[-1]))]
        assert y <= np.linalg.norm(V[-1]) + 1e-8


def test_convergence_bound_holds_for_every_leading_block(lz):
    """T_n is the Lanczos matrix of itself from e_1, so the Ritz value theta_k of its leading k x k block has residual
    b_k |y_k|: some eigenvalue of T_n lies that close to theta_k."""
    rng = np.random.RandomState(3)
    for trial in range(20):
        n = rng.randint(5, 80)
        a, b = rng.randn(n), rng.rand(n - 1) + 1e-3
        if trial % 4 == 0:
            b[rng.randint(0, n - 1)] = 0.0
        ev = np.linalg.eigvalsh(tri(a, b))
        for k in range(1, n):
            th = lz.max_eig(a[:k], b[:k - 1])
            y = lz.last_component(a[:k], b[:k - 1], th)
            bound = b[k - 1] * y
            assert np.min(np.abs(ev - th)) <= bound + 1e-12 * max(1.0, np.abs(ev).max()), (trial, k)
            assert th <= ev[-1] + 1e-12 * max(1.0, abs(ev[-1]))   # (Ritz values never pass the largest eigenvalue)


def test_convergence_bound_on_a_graph(lz):
    """On the Lanczos tridiagonal of a graph's adjacency, a Ritz value whose bound is met is the largest eigenvalue to that bound."""
    rng = np.random.RandomState(11)
    n = 120
    A = (rng.rand(n, n) < 0.05).astype(float)
    A = np.triu(A, 1)
    A = A + A.T
    lam = np.linalg.eigvalsh(A)[-1]
    al, be = lanczos_full(A, 60)
    hit = None
    for k in range(1, 61):
        th = lz.max_eig(al[:k], be[:k - 1])
        y = lz.last_component(al[:k], be[:k - 1], th)
        if lz.converged(be[k - 1], y, th, 1e-10):
            hit = k
            assert abs(th - lam) <= 1e-10 * lam
            break
    assert hit is not None


def test_converged_rule(lz):
    assert lz.converged(1e-3, 1e-8, 5.0, 1e-10)
    assert not lz.converged(1e-3, 1e-6, 5.0, 1e-10)
    assert lz.converged(0.0, 1.0, 0.0, 1e-10)


# ---------------------------------------------------------------- argument checks (host side, before any device call)
def _sc(m):
    return torch.zeros((m, 3), dtype=torch.float64)


@pytest.mark.parametrize("ptr", [[1, 4], [0, 3], [0, 5, 4], [0], [[0, 4]], [0.0, 4.0], "04"])
def test_bad_ptr_is_refused_before_any_device_call(ptr):
    from rlap_amd import ops
    with pytest.raises(ValueError):
        ops.snapshot_stats(_sc(4), ptr, 10)


def test_node_ptr_must_divide_the_segments():
    from rlap_amd import ops
    with pytest.raises(ValueError, match="divide"):
        ops.snapshot_stats(_sc(6), [0, 2, 4, 6], 10, node_ptr=[0, 5, 10])
    with pytest.raises(ValueError):
        ops.snapshot_stats(_sc(6), [0, 2, 4, 6], 10, node_ptr=[0, 5, 9])     # (does not end at num_nodes)
    with pytest.raises(ValueError):
        ops.snapshot_stats(_sc(6), [0, 2, 4, 6], 10, node_ptr=[0, 6, 5, 10])  # (decreasing)


@pytest.mark.parametrize("kw", [{"tol": 0.0}, {"tol": -1e-3}, {"tol": float("nan")}, {"max_iter": 0}, {"max_iter": 5000},
                                {"max_iter": 2.5}])
def test_bad_tolerances_are_refused(kw):
    from rlap_amd import ops
    with pytest.raises(ValueError):
        ops.snapshot_stats(_sc(4), [0, 4], 10, **kw)


def test_bad_sc_and_num_nodes_are_refused():
    from rlap_amd import ops
    with pytest.raises(ValueError):
        ops.snapshot_stats(torch.zeros((4, 2), dtype=torch.float64), [0, 4], 10)
    with pytest.raises(ValueError):
        ops.snapshot_stats(_sc(4), [0, 4], -1)

