// rlap_lanczos.h -- the tridiagonal half of the snapshot statistics' Lanczos iteration (rlap_stats.hip): Sturm
// counts, bisection for the largest eigenvalue of T_k, the last component of its eigenvector and the convergence test.
// Plain __host__ __device__ functions without any HIP dependency: tests/test_snapshot_stats_cpu.py compiles this file with g++.
//
// T_k is symmetric tridiagonal: diagonal a[0..k), off-diagonal b[0..k-1) (b[i] couples rows i and i+1).
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RLAP_LZ_HD __host__ __device__ inline
#else
#define RLAP_LZ_HD inline
#endif

namespace rlap {
namespace lanczos {

// smallest pivot magnitude the Sturm recurrence lets through (LAPACK dstebz's pivmin)
RLAP_LZ_HD double pivmin(const double* b, int k) {
    double m = 1.0;
    for (int i = 0; i + 1 < k; ++i) m = fmax(m, b[i] * b[i]);
    return DBL_MIN * m;
}

// number of eigenvalues of T_k below x: negative pivots of the LDL^T factorisation of T_k - x I
RLAP_LZ_HD int count_below(const double* a, const double* b, int k, double x, double pmin) {
    int c = 0;
    double d = 1.0;
    for (int i = 0; i < k; ++i) {
        d = (a[i] - x) - (i > 0 ? (b[i - 1] * b[i - 1]) / d : 0.0);
        if (fabs(d) <= pmin) d = -pmin;
        c += d < 0.0 ? 1 : 0;
    }
    return c;
}

// bracket [lo, hi] of the spectrum (Gershgorin discs), widened so that count_below(hi) == k and count_below(lo) == 0
RLAP_LZ_HD void bracket(const double* a, const double* b, int k, double* lo, double* hi) {
    double l = a[0], h = a[0], nrm = 0.0;
    for (int i = 0; i < k; ++i) {
        const double r = (i > 0 ? fabs(b[i - 1]) : 0.0) + (i + 1 < k ? fabs(b[i]) : 0.0);
        l = fmin(l, a[i] - r);
        h = fmax(h, a[i] + r);
        nrm = fmax(nrm, fabs(a[i]) + r);
    }
    const double pad = 4.0 * DBL_EPSILON * nrm * k + 2.0 * pivmin(b, k);
    *lo = l - pad;
    *hi = h + pad;
}

// largest eigenvalue of T_k by bisection to full precision: the invariant is count_below(lo) < k == count_below(hi); the loop
// stops when no double lies strictly between lo and hi (at most ~2100 halvings for the widest finite bracket; 128 suffice here)
RLAP_LZ_HD double max_eig(const double* a, const double* b, int k) {
    if (k == 1) return a[0];
    const double pm = pivmin(b, k);
    double lo, hi;
    bracket(a, b, k, &lo, &hi);
    for (int it = 0; it < 2200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi)) break;
        if (count_below(a, b, k, mid, pm) == k) hi = mid; else lo = mid;
    }
    return hi;
}

// |y_{k-1}|: the last component of the unit eigenvector y of T_k for its eigenvalue theta, by the twisted factorisation
// (T - theta) = N_r D_r N_r^T (Dhillon): forward pivots dp[i] (the Sturm pivots at theta) and backward pivots dm[i] meet at the
// twist index r where |gamma_r| is least, i.e. where the eigenvector is largest; from z_r = 1 the components are built outwards,
// each a product of ratios b / pivot that shrink away from r -- stable whether the vector sits at the top of T (a converged
// Ritz vector, tiny last component) or at the bottom.  A zero off-diagonal cuts the products: a vector living in a block above
// the last split has last component 0.  dp, dm: scratch of k doubles each.
RLAP_LZ_HD double last_component(const double* a, const double* b, int k, double theta, double* dp, double* dm) {
    if (k == 1) return 1.0;
    const double pm = pivmin(b, k);
    double d = 0.0;
    for (int i = 0; i < k; ++i) {
        d = (a[i] - theta) - (i > 0 ? (b[i - 1] * b[i - 1]) / d : 0.0);
        if (fabs(d) <= pm) d = -pm;
        dp[i] = d;
    }
    for (int i = k - 1; i >= 0; --i) {
        d = (a[i] - theta) - (i + 1 < k ? (b[i] * b[i]) / d : 0.0);
        if (fabs(d) <= pm) d = -pm;
        dm[i] = d;
    }
    int r = 0;
    double gmin = INFINITY;
    for (int i = 0; i < k; ++i) {
        const double g = fabs(dp[i] + dm[i] - (a[i] - theta));
        if (g < gmin) { gmin = g; r = i; }
    }
    double ss = 1.0, z = 1.0;
    for (int i = r - 1; i >= 0; --i) { z = -b[i] * z / dp[i]; ss += z * z; }
    z = 1.0;
    for (int i = r + 1; i < k; ++i) { z = -b[i - 1] * z / dm[i]; ss += z * z; }
    return fabs(z) / sqrt(ss);
}

// the stopping rule: the Ritz pair (theta, V y) of T_j has residual ||A V y - theta V y|| = beta_j |y_j|, so some eigenvalue of A
// lies within beta_j |y_j| of theta; stop when that is at most tol * |theta|
RLAP_LZ_HD bool converged(double beta, double ylast, double theta, double tol) {
    return beta * ylast <= tol * fabs(theta);
}

}  // namespace lanczos
}  // namespace rlap
