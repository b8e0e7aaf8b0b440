// rlap_cheb.h -- the fixed-step Chebyshev iteration of the PPR diffusion (rlap_snapshot_ppr, rlap_ppr.hip): the step
// count and the recurrence coefficients.  Plain __host__ __device__ functions without any HIP dependency: tests/test_ppr_cpu.py
// compiles this file with g++ and runs the recurrence on dense matrices.
//
// The system is M x = alpha e_j with M = I - B, B = (1 - alpha) Â (Â = D^-1/2 A D^-1/2, or with A + I).  The spectrum of Â lies in
// [-1, 1], so that of B lies in [-rho, rho] with rho = 1 - alpha.  Chebyshev semi-iteration for x = B x + f (f = alpha e_j) from
// x_0 = 0:
//     x_1 = f,     x_{k+1} = omega_{k+1} (B x_k + f - x_{k-1}) + x_{k-1},     omega_{k+1} = 2 mu T_k(mu) / T_{k+1}(mu),  mu = 1 / rho
// has error x - x_K = [T_K(B / rho) / T_K(mu)] (x - x_0), so ||x - x_K||_2 <= ||x||_2 / T_K(mu) <= 1 / T_K(mu) (||S e_j||_2 <= 1).
// The step count is the least K with T_K(mu) >= 1 / tol; no dot product, no data-dependent stop.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RLAP_CH_HD __host__ __device__ inline
#else
#define RLAP_CH_HD inline
#endif

namespace rlap {
namespace cheb {

constexpr int MAX_STEPS = 4096;   // cap on K (at tol = 1e-10: alpha = 0.2 needs 35, alpha = 1e-3 531, alpha = 1e-4 1,678)

// K = min{K >= 0 : T_K(1 / (1 - alpha)) >= 1 / tol} with T_K by its three-term recurrence, or -1 when 0 < alpha < 1 and tol > 0
// do not hold or K would exceed `cap`
RLAP_CH_HD int steps(double alpha, double tol, int cap) {
    if (!(alpha > 0.0 && alpha < 1.0) || !(tol > 0.0)) return -1;
    const double mu = 1.0 / (1.0 - alpha), goal = 1.0 / tol;
    double tp = 1.0, t = mu;   // T_{k-1}, T_k
    if (1.0 >= goal) return 0;
    for (int k = 1; k <= cap; ++k) {
        if (t >= goal) return k;
        const double tn = 2.0 * mu * t - tp;
        tp = t; t = tn;
    }
    return -1;
}

// om[k] (1 <= k < K): the weight of the step that makes x_{k+1} from x_k and x_{k-1}; om[0] = 1 (x_1 = f)
RLAP_CH_HD void omegas(double alpha, int K, double* om) {
    const double mu = 1.0 / (1.0 - alpha);
    double tp = 1.0, t = mu;
    if (K > 0) om[0] = 1.0;
    for (int k = 1; k < K; ++k) {
        const double tn = 2.0 * mu * t - tp;
        om[k] = 2.0 * mu * t / tn;
        tp = t; t = tn;
    }
}

// one entry of one step: y = (B x_k + f) at that entry, xp = x_{k-1} there; returns x_{k+1}
RLAP_CH_HD double step(double om, double y, double xp) { return om * (y - xp) + xp; }

}  // namespace cheb
}  // namespace rlap
