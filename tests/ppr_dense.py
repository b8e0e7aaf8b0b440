"""The dense float64 reference of the PPR diffusion (ops.snapshot_ppr) for the GPU tests: one segment's
S = alpha (I - (1 - alpha) D^-1/2 A D^-1/2)^-1 by numpy.linalg.inv, thresholded and normalised as adapters.compute_ppr does, and a
device result scattered into the same dense layout."""
import numpy as np
import torch


def _numpy(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def system(part, weighted=True, self_loop=False):
    """(sorted ids, D^-1/2 A D^-1/2) of one segment's rows [i, j, w]: duplicates summed, A + I with self_loop, 0 for a zero degree."""
    part = _numpy(part)
    nodes = np.unique(part[:, :2].astype(np.int64))
    k = len(nodes)
    A = np.zeros((k, k))
    r = np.searchsorted(nodes, part[:, 0].astype(np.int64))
    c = np.searchsorted(nodes, part[:, 1].astype(np.int64))
    np.add.at(A, (r, c), part[:, 2] if weighted else 1.0)
    if self_loop:
        A += np.eye(k)
    d = A.sum(1)
    dinv = np.where(d > 0, d ** -0.5, 0)
    return nodes, dinv[:, None] * A * dinv[None, :]


def dense_ppr(part, alpha=0.2, eps=1e-4, weighted=True, self_loop=False, normalize=True):
    """(nodes, S before threshold, S kept (and normalised)) of one segment in float64 numpy (the formula of test_ppr_diffusion_adapter)."""
    nodes, Ahat = system(part, weighted, self_loop)
    S0 = alpha * np.linalg.inv(np.eye(len(nodes)) - (1 - alpha) * Ahat)
    return nodes, S0, threshold(S0, eps, normalize)


def chebyshev_iterates(Ahat, alpha, K):
    """(x_{K-1}, x_K) of the recurrence of rlap_amd/csrc/rlap_cheb.h for all sources at once, dense (K >= 1): x_0 = 0, x_1 = alpha I,
    x_{k+1} = om_{k+1} (B x_k + alpha I - x_{k-1}) + x_{k-1} with B = (1 - alpha) Ahat, om_{k+1} = 2 mu T_k(mu) / T_{k+1}(mu),
    mu = 1 / (1 - alpha).  Ahat: a numpy array, or a float64 torch tensor (the products then run where it lives); returns numpy."""
    k = Ahat.shape[0]
    eye = np.eye(k) if isinstance(Ahat, np.ndarray) else torch.eye(k, dtype=Ahat.dtype, device=Ahat.device)
    F = alpha * eye
    B = (1.0 - alpha) * Ahat
    mu = 1.0 / (1.0 - alpha)
    xp, x = 0.0 * eye, 1.0 * F
    tp, t = 1.0, mu
    for _ in range(1, K):
        tn = 2.0 * mu * t - tp
        om = 2.0 * mu * t / tn
        xp, x = x, om * (B @ x + F - xp) + xp
        tp, t = t, tn
    return _numpy(xp), _numpy(x)


def threshold(S0, eps, normalize=True):
    """The entries >= eps of S0, then (normalize) D_S^-1/2 S D_S^-1/2 with D_S the row sums of what was kept."""
    S = np.where(S0 >= eps, S0, 0.0)
    if normalize:
        d2 = S.sum(1)
        d2inv = np.where(d2 > 0, d2 ** -0.5, 0)
        S = d2inv[:, None] * S * d2inv[None, :]
    return S


def to_dense(out, nodes):
    """(values, pattern) of output rows [i, j, value] as dense (k, k) arrays over the sorted ids `nodes`; every (i, j) occurs once."""
    o = _numpy(out)
    k = len(nodes)
    i = np.searchsorted(nodes, o[:, 0].astype(np.int64))
    j = np.searchsorted(nodes, o[:, 1].astype(np.int64))
    assert i.size == 0 or (i.max() < k and j.max() < k)
    assert np.array_equal(nodes[i], o[:, 0]) and np.array_equal(nodes[j], o[:, 1]), "an output id is not an id of the segment"
    flat = i * k + j
    assert np.unique(flat).size == flat.size, "an (i, j) pair occurs twice"
    D = np.zeros((k, k))
    keep = np.zeros((k, k), dtype=bool)
    D.ravel()[flat] = o[:, 2]
    keep.ravel()[flat] = True
    return D, keep
