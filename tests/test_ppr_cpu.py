"""PPR diffusion without a GPU: the step count and the Chebyshev recurrence of rlap_amd/csrc/rlap_cheb.h (compiled here with g++,
the same source rlap_ppr.hip includes) against numpy, and the host-side argument checks of ops.snapshot_ppr / ops.ppr_diffusion."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from util import ba_graph, grid2d, path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "rlap_amd", "csrc", "rlap_cheb.h")

WRAP = r"""
#include <vector>
#include "rlap_cheb.h"
extern "C" {
int ch_steps(double alpha, double tol, int cap) { return rlap::cheb::steps(alpha, tol, cap); }
int ch_max_steps() { return rlap::cheb::MAX_STEPS; }
// x_K of M x = alpha e_j, M = I - (1 - alpha) Ahat, Ahat dense n x n (row-major), by the header's recurrence
void ch_solve(const double* ahat, int n, double alpha, int K, int j, double* x) {
    std::vector<double> om(K > 0 ? K : 1), cur(n, 0.0), prv(n, 0.0), y(n);
    rlap::cheb::omegas(alpha, K, om.data());
    if (K > 0) cur[j] = alpha;
    for (int k = 1; k < K; ++k) {
        for (int i = 0; i < n; ++i) {
            double acc = 0.0;
            for (int c = 0; c < n; ++c) acc += (1.0 - alpha) * ahat[(size_t)i * n + c] * cur[c];
            y[i] = acc + (i == j ? alpha : 0.0);
        }
        for (int i = 0; i < n; ++i) prv[i] = rlap::cheb::step(om[k], y[i], prv[i]);
        std::swap(cur, prv);
    }
    for (int i = 0; i < n; ++i) x[i] = cur[i];
}
}
"""


@pytest.fixture(scope="module")
def ch(tmp_path_factory):
    d = tmp_path_factory.mktemp("cheb")
    src, so = d / "ch.cc", d / "libch.so"
    src.write_text(WRAP)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.dirname(HDR),
                           "-o", str(so), str(src)])
    lib = ctypes.CDLL(str(so))
    cd, ci, dp = ctypes.c_double, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
    lib.ch_steps.restype = ci
    lib.ch_steps.argtypes = [cd, cd, ci]
    lib.ch_max_steps.restype = ci
    lib.ch_solve.restype = None
    lib.ch_solve.argtypes = [dp, ci, cd, ci, ci, dp]
    return lib


def cheb_T(k, mu):
    """T_k(mu) for mu >= 1 in closed form."""
    return math.cosh(k * math.acosh(mu))


@pytest.mark.parametrize("alpha", [0.05, 0.1, 0.15, 0.2, 0.5, 0.9])
@pytest.mark.parametrize("tol", [1e-4, 1e-8, 1e-10, 1e-12, 1e-14])
def test_step_count_is_least(ch, alpha, tol):
    K = ch.ch_steps(alpha, tol, ch.ch_max_steps())
    mu = 1.0 / (1.0 - alpha)
    assert K >= 1
    # least K with T_K(mu) >= 1/tol: the closed form agrees on both sides (a relative margin for rounding at the boundary)
    assert cheb_T(K, mu) >= (1.0 / tol) * (1 - 1e-9)
    assert cheb_T(K - 1, mu) < (1.0 / tol) * (1 + 1e-9)
    from rlap_amd import ops
    assert ops.ppr_steps(alpha, tol) == K


def test_step_count_defaults_and_cap(ch):
    assert ch.ch_steps(0.2, 1e-10, 4096) == 35          # cosh(K ln 2) >= 1e10
    assert ch.ch_steps(0.2, 1e-12, 4096) == 41
    assert ch.ch_steps(0.2, 2.0, 4096) == 0             # T_0 = 1 >= 1/tol
    assert ch.ch_steps(1e-4, 1e-10, 4096) == 1678
    assert ch.ch_steps(1e-4, 1e-10, 1000) == -1         # over the cap
    assert ch.ch_steps(0.0, 1e-10, 4096) == -1 and ch.ch_steps(1.0, 1e-10, 4096) == -1 and ch.ch_steps(0.2, 0.0, 4096) == -1


def ahat_of(ei, n, w=None, self_loop=False):
    A = np.zeros((n, n))
    np.add.at(A, (ei[0], ei[1]), 1.0 if w is None else w)
    if self_loop:
        A += np.eye(n)
    d = A.sum(1)
    dinv = np.where(d > 0, d ** -0.5, 0.0)
    return dinv[:, None] * A * dinv[None, :]


def random_graph(n, p, seed):
    rs = np.random.RandomState(seed)
    U = np.triu(rs.rand(n, n) < p, 1)
    r, c = np.nonzero(U)
    w = rs.uniform(0.5, 2.0, r.size)
    return np.stack([np.concatenate([r, c]), np.concatenate([c, r])]), np.concatenate([w, w])


GRAPHS = {
    "random": lambda: random_graph(60, 0.08, 3),
    "path": lambda: (path(40), None),
    "grid": lambda: (grid2d(6, 7), None),     # bipartite: the spectrum of Ahat reaches -1
    "ba": lambda: (ba_graph(50, 3, 1), None),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("self_loop", [False, True])
@pytest.mark.parametrize("alpha,tol", [(0.2, 1e-10), (0.1, 1e-12), (0.5, 1e-8)])
def test_recurrence_meets_the_bound(ch, name, self_loop, alpha, tol):
    ei, w = GRAPHS[name]()
    ei = np.asarray(ei, dtype=np.int64)
    n = int(ei.max()) + 1
    ah = np.ascontiguousarray(ahat_of(ei, n, w, self_loop))
    ev = np.linalg.eigvalsh(ah)
    assert ev.min() >= -1 - 1e-12 and ev.max() <= 1 + 1e-12
    if name == "grid" and not self_loop:
        assert ev.min() < -1 + 1e-9                     # the bound is tight at -1 here
    M = np.eye(n) - (1 - alpha) * ah
    S = alpha * np.linalg.inv(M)
    K = ch.ch_steps(alpha, tol, 4096)
    x = np.zeros(n)
    dp = ctypes.POINTER(ctypes.c_double)
    for j in (0, n // 2, n - 1):
        ch.ch_solve(ah.ctypes.data_as(dp), n, alpha, K, j, x.ctypes.data_as(dp))
        assert np.abs(x - S[:, j]).max() <= tol
        assert np.linalg.norm(S[:, j]) <= 1 + 1e-12
    # one step fewer does not meet the bound on every column in general; with K it always does (above)


# ---------------------------------------------------------------- host-side argument checks (nothing is launched: no GPU here)
SC = torch.tensor([[1.0, 0.0, 1.0], [0.0, 1.0, 1.0]], dtype=torch.float64)


@pytest.mark.parametrize("kw", [
    {"alpha": 0.0}, {"alpha": 1.0}, {"alpha": -0.1}, {"alpha": float("nan")}, {"alpha": True},
    {"eps": 0.0}, {"eps": -1e-4}, {"eps": float("nan")},
    {"tol": 0.0}, {"tol": -1.0}, {"tol": float("inf")},
    {"alpha": 1e-4, "tol": 1e-10},          # K = 1,678 <= 4,096: allowed ...
])
def test_snapshot_ppr_bad_params(kw):
    from rlap_amd import ops
    if kw == {"alpha": 1e-4, "tol": 1e-10}:
        assert ops.ppr_steps(1e-4, 1e-10) == 1678
        kw = {"alpha": 1e-5, "tol": 1e-10}  # ... but K = 5,300 is over the cap
    with pytest.raises(ValueError):
        ops.snapshot_ppr(SC, [0, 2], 2, **kw)
    with pytest.raises(ValueError):
        ops.ppr_diffusion(SC[:, :2].long().t(), None, 2, **kw)


@pytest.mark.parametrize("args,kw", [
    ((SC, [0, 3], 2), {}),                               # ptr[-1] != rows
    ((SC, [1, 2], 2), {}),                               # ptr[0] != 0
    ((SC, [0, 2, 1, 2], 2), {}),                         # decreasing
    ((SC, [0, 2], -1), {}),                              # num_nodes
    ((SC[:, :2], [0, 2], 2), {}),                        # not (m, 3)
    ((SC, [0, 1, 2], 2), {"node_ptr": [0, 1, 2, 2]}),   # 3 graphs do not divide 2 segments
    ((SC, [0, 2], 2), {"node_ptr": [0, 1]}),            # node_ptr[-1] != num_nodes
    ((torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=torch.float64), [0, 2], 2), {}),    # weight 0
    ((torch.tensor([[1.0, 0.0, -1.0], [0.0, 1.0, -1.0]], dtype=torch.float64), [0, 2], 2), {}),  # negative weight
])
def test_snapshot_ppr_bad_tables(args, kw):
    from rlap_amd import ops
    with pytest.raises(ValueError):
        ops.snapshot_ppr(*args, **kw)


def test_ppr_diffusion_bad_input():
    from rlap_amd import ops
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(ValueError):
        ops.ppr_diffusion(ei, torch.tensor([1.0, -1.0], dtype=torch.float64), 2)     # negative weight
    with pytest.raises(ValueError):
        ops.ppr_diffusion(ei, torch.tensor([1.0]), 2)                                 # one weight per edge
    with pytest.raises(ValueError):
        ops.ppr_diffusion(ei, None, 1)                                                # id out of range
    with pytest.raises(ValueError):
        ops.ppr_diffusion(ei[0], None, 2)                                             # not (2, E)
    with pytest.raises(ValueError):
        ops.ppr_diffusion(ei, None, -2)
