// rlap_cca.h -- the rule of the fused CCA-SSG loss (rlap_cca_loss / rlap_cca_loss_backward, rlap_cca.hip): every value
// of the call and the order of every sum.  Plain __host__ __device__ functions without any HIP dependency, as rlap_infonce.h:
// tests/csrc/cca_mirror.cc compiles this file with g++ (contraction off, as the library) and computes the same bits;
// tests/csrc/cca_main.cc runs the index arithmetic under the sanitizers; the kernels read the same functions.
//
// Inputs: h1 and h2, (N, F) float32, 2 <= N < 2^31, 1 <= F <= 512, and lambd finite and >= 0.  With z = (h - mean_0(h)) / std_0(h)
// (the unbiased deviation), c = z1^T z2 / N, c1 = z1^T z1 / N, c2 = z2^T z2 / N the loss is
// -trace(c) + lambd * (||I - c1||_F^2 + ||I - c2||_F^2).  "The chunk rule" below is rlap_spmm.h's: the terms c_e * x_e of a list
// (product rounded, add rounded, float64) summed from 0 in chunks of 256 in order, the chunk sums added to 0 in order.
//
//   column stats    mean_k = (chunk rule over i of 1 * (double)h_ik) / N;  ss_k = chunk rule over i of d * d, d = (double)h_ik - mean_k;
//                   sd_k = sqrt(ss_k / (N - 1));  z_ik = (float)(((double)h_ik - mean_k) / sd_k).  A column of zero variance divides by
//                   zero, as in the reference: its z is NaN, and so are the loss and the gradients.  Nothing is clamped.
//   Gram sums       for k <= l:  S1_kl = 0 + part 0 + part 1 + ... in float64, a part being the float32 fmaf chain over its rows i in
//                   increasing order from +0: acc = fmaf(z1_ik, z1_il, acc) -- what v_mfma_f32_32x32x2_f32 computes with the node
//                   index as k.  The parts are the row ranges [part_begin(N, F, p), part_begin(N, F, p + 1)), multiples of 32 rows,
//                   a function of (N, F) alone; the last one ends at the padded row count, and a row >= N takes its turn as
//                   fmaf(0, 0, acc).  S1_lk = S1_kl (the product commutes, so the chain of (l, k) has the same bits anyway).  The
//                   sign of a zero S reaches no result: S enters only as delta - S / N.
//   residual        R1_kl = delta_kl - S1_kl / N in float64;  r1_kl = (float)R1_kl (the call's `gram` result, exactly symmetric).
//   loss terms      dec1 = chunk rule over the F * F entries of R1 in row-major order of R * R;  d_k = chunk rule over i of
//                   (double)z1_ik * (double)z2_ik;  inv = -(chunk rule over k of 1 * d_k) / N;  loss = inv + lambd * (dec1 + dec2).
//   backward        with the upstream gradient g:  P1_ik = the float32 fmaf chain over l = 0 .. F-1 in increasing order from +0 of
//                   fmaf(z1_il, r1_lk, acc); the kernel runs on over the zero columns up to the next multiple of 32, each
//                   fmaf(0, 0, acc), which can only turn a -0 into +0, and the sign of a zero P reaches dz only as the sign of a zero.
//                   dz1_ik = g * (-(double)z2_ik / N - ((4 lambd) / N) * (double)P1_ik);
//                   m_k = (chunk rule over i of 1 * dz1_ik) / N;  q_k = (chunk rule over i of dz1_ik * (double)z1_ik) / (N - 1);
//                   dh1_ik = (float)(((dz1_ik - m_k) - (double)z1_ik * q_k) / sd1_k).  dh2 is the same with the roles swapped.
//                   dz is a function of stored float32 values and is formed again wherever it is read; it is never stored.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rlap_spmm.h"
#include "rlap_tile32.h"

namespace rlap {
namespace cca {

// a Gram tile is rlap_tile32.h's: its sizes and its register layout (reg_row)
using tile32::TILE;
using tile32::num_tiles;
using tile32::padded_rows;
using tile32::feature_tiles;
using tile32::padded_features;
using tile32::reg_row;

constexpr int MAX_F = 512;                // feature columns of a call
constexpr int SUPER = 2;                  // a wave owns SUPER x SUPER Gram tiles: a 64 x 64 "super tile" pair
constexpr int GROUP_PAIRS = 4;            // super-tile pairs of a workgroup (one per wave)
constexpr int64_t TARGET_GROUPS = 256;    // workgroups a view aims at: what num_parts() is made from
constexpr int64_t MAX_PARTS = 64;         // (bounds the part accumulators of the arena)

RLAP_SPMM_HD bool lambd_ok(double l) { return l >= 0.0 && l <= 1.7976931348623157e308; }   // (false for a NaN and for inf)

// the 64-column tiles of F columns
RLAP_SPMM_HD int super_tiles(int64_t F) { return (feature_tiles(F) + SUPER - 1) / SUPER; }
// the upper triangle of super-tile pairs (I <= J), numbered row by row, and the workgroups of a (view, part) that share them out
RLAP_SPMM_HD int super_pairs(int64_t F) { return super_tiles(F) * (super_tiles(F) + 1) / 2; }
RLAP_SPMM_HD int pair_groups(int64_t F) { return (super_pairs(F) + GROUP_PAIRS - 1) / GROUP_PAIRS; }
RLAP_SPMM_HD void pair_of(int q, int nst, int* I, int* J) {   // 0 <= q < nst (nst + 1) / 2
    int i = 0;
    while (q >= nst - i) { q -= nst - i; ++i; }
    *I = i; *J = i + q;
}
// tile a (0 or 1) of super tile I, kept inside the nft tiles of the image (a clamped tile is computed twice and stored once)
RLAP_SPMM_HD int tile_of(int I, int a, int nft) { const int t = SUPER * I + a; return t < nft ? t : nft - 1; }
// whether the wave of pair (I, J) stores its tile (a, b): inside the image and in the upper triangle of tiles
RLAP_SPMM_HD bool tile_stored(int I, int J, int a, int b, int nft) {
    const int tk = SUPER * I + a, tl = SUPER * J + b;
    return tk < nft && tl < nft && tk <= tl;
}

// Which instances the launchers of rlap_cca.hip take for nft = feature_tiles(F); 0 for an nft outside [1, MAX_F / TILE], which no
// launcher accepts.
//   k_cca_gram<NV>   a thread stages nft float4s of a 32-row step and guards each with j < nft: the ladder's instance.
//   k_cca_zr<NCT>    wave w owns the column tiles w, w + 4, ..., guarded with w + 4 j < nft: NCT = ceil(nft / 4), 1 to 4.
static_assert(MAX_F / TILE == tile32::MAX_INSTANCE, "the ladder ends at MAX_F");
RLAP_SPMM_HD int gram_instance(int nft) { return tile32::ladder_instance(nft); }
RLAP_SPMM_HD int zr_instance(int nft) {
    if (nft < 1 || nft > MAX_F / TILE) return 0;
    return (nft + 3) / 4;   // (four waves a workgroup)
}

// The parts of the rows: a function of (N, F) alone. As many as bring a view's pair groups up to TARGET_GROUPS workgroups, at most
// one per 32-row tile and at most MAX_PARTS.
RLAP_SPMM_HD int64_t num_parts(int64_t N, int64_t F) {
    const int64_t T = num_tiles(N), G = pair_groups(F);
    if (T < 1 || G < 1) return 1;
    int64_t p = (TARGET_GROUPS + G - 1) / G;
    if (p > MAX_PARTS) p = MAX_PARTS;
    return p < 1 ? 1 : (p > T ? T : p);
}
RLAP_SPMM_HD int64_t part_begin(int64_t N, int64_t F, int64_t p) { return (p * num_tiles(N) / num_parts(N, F)) * TILE; }   // a ROW; (T < 2^26, p <= 64)

// ---- the values
RLAP_SPMM_HD double col_mean(double total, int64_t N) { return total / (double)N; }
RLAP_SPMM_HD double centred(float h, double mean) { return (double)h - mean; }
RLAP_SPMM_HD double col_sd(double ss, int64_t N) { return sqrt(ss / (double)(N - 1)); }
RLAP_SPMM_HD float zval(float h, double mean, double sd) { return (float)(centred(h, mean) / sd); }

RLAP_SPMM_HD float gram_step(float acc, float x, float y) { return fmaf(x, y, acc); }
RLAP_SPMM_HD double resid(double S, int64_t N, bool diagonal) { return (diagonal ? 1.0 : 0.0) - S / (double)N; }
RLAP_SPMM_HD double inv_of(double dsum, int64_t N) { return -dsum / (double)N; }
RLAP_SPMM_HD double loss_of(double inv, double lambd, double dec1, double dec2) {
    const double t = dec1 + dec2;
    const double u = lambd * t;
    return inv + u;
}

RLAP_SPMM_HD double coef4(double lambd, int64_t N) { return (4.0 * lambd) / (double)N; }
// the gradient with respect to a standardised element: `other` is the element of the other view, P the chain's sum
RLAP_SPMM_HD double dz_of(double g, float other, float P, int64_t N, double c4) {
    const double t = -(double)other / (double)N;
    const double u = c4 * (double)P;
    return g * (t - u);
}
RLAP_SPMM_HD double col_m(double total, int64_t N) { return total / (double)N; }
RLAP_SPMM_HD double col_q(double total, int64_t N) { return total / (double)(N - 1); }
RLAP_SPMM_HD float dh_of(double dz, double m, float z, double q, double sd) {
    const double a = dz - m;
    const double b = (double)z * q;
    return (float)((a - b) / sd);
}

// the chunk rule over n terms c(e) * x(e)
template <class Coef, class Feat>
RLAP_SPMM_HD double rule_sum(int64_t n, Coef c, Feat x) { return spmm::list_sum(n, c, x, false, 0.0, 0.0); }

}  // namespace cca
}  // namespace rlap
