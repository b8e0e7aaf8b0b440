// rlap_markov.h -- the scalar rule of the Markov diffusion (rlap_snapshot_markov, rlap_markov.hip): every floating-point
// step of one column, written once.  Plain __host__ __device__ functions without any HIP dependency: tests/csrc/markov_mirror.cc
// compiles this file with g++ and, the library being built with -ffp-contract=off, computes the device's bits.
//
// With Â = D^-1/2 A D^-1/2 (or with A + I), beta = 1 - alpha and order D >= 1 the diffusion is
//     M = alpha Â + (1/D) sum_{k=0..D} beta^k Â^(k+1)
// (the published loop: z = Â; t = Â; D times: t = beta Â t, z += t; z /= D; z += alpha Â).  Column j in Horner form:
//     h_0 = e_j,   h_{m+1} = e_j + beta (Â h_m)  (m = 0 .. D-1),   u = alpha e_j + h_D / D,   M e_j = Â u
// -- D + 1 applications of Â on two copies of the column.  An application at node i sums coef_r * x[node of row r] over the rows of
// i's block in row order (duplicates in input order), then adds diag_i * x[i] (the self loop; the term is added also where it is 0).
// h_0 lies in copy 0; application m reads copy m & 1 and writes the other one; the u step is applied to the entry an application
// m = D - 1 writes, in place; the last application (m = D) therefore leaves M e_j in copy final_copy(D).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RLAP_MK_HD __host__ __device__ inline
#else
#define RLAP_MK_HD inline
#endif

namespace rlap {
namespace markov {

constexpr int MAX_ORDER = 1024;   // cap on the order D

// the parameter rule of the call
RLAP_MK_HD bool valid(double alpha, int order, double eps) {
    return alpha >= 0.0 && alpha <= 1.0 && order >= 1 && order <= MAX_ORDER && eps > 0.0 && eps < INFINITY;
}

// D^-1/2 of a degree (0 for a zero degree)
RLAP_MK_HD double dinv(double d) { return d > 0.0 ? 1.0 / sqrt(d) : 0.0; }
// the stored coefficient of a row of weight w between nodes of D^-1/2 di and dj
RLAP_MK_HD double coef(double w, double di, double dj) { return w * (di * dj); }
// the diagonal term of the self loop
RLAP_MK_HD double diag(double di) { return di * di; }

// one entry of application m < D: acc = (Â h_m) there, src: the entry is the source's own.  The last of them (m = D - 1) goes on
// to u.
RLAP_MK_HD double horner(double acc, bool src, double beta) {
    const double t = beta * acc;
    return src ? 1.0 + t : t;
}
RLAP_MK_HD double ustep(double h, bool src, double alpha, int order) {
    const double q = h / (double)order;
    return src ? alpha + q : q;
}
RLAP_MK_HD double step(double acc, bool src, double alpha, double beta, int order, int m) {
    const double h = horner(acc, src, beta);
    return m == order - 1 ? ustep(h, src, alpha, order) : h;
}
// one entry of the last application (m = D): M_ij itself
RLAP_MK_HD double last(double acc) { return acc; }

RLAP_MK_HD double beta_of(double alpha) { return 1.0 - alpha; }
// which copy holds M e_j after the D + 1 applications
RLAP_MK_HD int final_copy(int order) { return (order & 1) ? 0 : 1; }

}  // namespace markov
}  // namespace rlap
