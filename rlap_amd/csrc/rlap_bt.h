// rlap_bt.h -- the rule of the fused Barlow Twins loss (rlap_bt_loss / rlap_bt_loss_backward, rlap_bt.hip): every value
// of the call and the order of every sum.  Plain __host__ __device__ functions without any HIP dependency, as rlap_cca.h:
// tests/csrc/bt_mirror.cc compiles this file with g++ (contraction off, as the library) and computes the same bits;
// tests/csrc/bt_main.cc runs the index arithmetic under the sanitizers; the kernels read the same functions.  Where a value is
// rlap_cca.h's or rlap_tile32.h's it is that function, not a copy of it.
//
// Inputs: h1 and h2, (N, F) float32, 2 <= N < 2^31, 1 <= F <= 512; lambd and eps finite and >= 0; flags bit 0 (NO_STANDARDIZE): z = h.
// With z = (h - mean_0(h)) / (std_0(h) + eps) (the unbiased deviation) and c = z1^T z2 / N the loss is
// sum_k (1 - c_kk)^2 + lambd * sum_{k != l} c_kl^2 -- the published bt_loss of PyGCL's L.BarlowTwins.  "The chunk rule" is
// rlap_spmm.h's, as in rlap_cca.h.
//
//   column stats    mean_k, ss_k, sd_k: rlap_cca.h's, by the same functions and the same chunk rule;
//                   z_ik = (float)(((double)h_ik - mean_k) / (sd_k + eps)): with eps = 0 cca::zval bit for bit (sd + 0 is sd).
//                   With NO_STANDARDIZE z = h, no statistics are taken and colstat is neither written nor read.
//   cross sums      for EVERY (k, l):  S_kl = 0 + part 0 + part 1 + ... in float64, a part being the float32 fmaf chain over its
//                   rows i in increasing order from +0: acc = fmaf(z1_ik, z2_il, acc) -- what v_mfma_f32_32x32x2_f32 computes with
//                   the node index as k.  The parts are the row ranges [part_begin(N, F, p), part_begin(N, F, p + 1)), multiples
//                   of 32 rows, a function of (N, F) alone; a row >= N takes its turn as fmaf(0, 0, acc).
//   loss terms      c_kl = S_kl / N in float64;  cross_kl = (float)c_kl (the call's (F, F) row-major result, which the backward
//                   reads);  on = chunk rule over k of d * d, d = 1 - c_kk;  off = chunk rule over the F * F entries in row-major
//                   order of o * o, o = c_kl off the diagonal and 0 on it;  loss = on + lambd * off.
//   backward        from stored float32 values only.  W_kl = (float)(k == l ? -2 (1 - (double)cross_kk) : (2 lambd) (double)cross_kl);
//                   P1_ik = the float32 fmaf chain over l = 0 .. F-1 in increasing order from +0 of fmaf(z2_il, W_kl, acc) and
//                   P2_ik that of fmaf(z1_il, W_lk, acc) -- the z r product of rlap_cca.h with W^T and W as its B operand; the
//                   kernel runs on over the zero columns up to the next multiple of 32, as there.
//                   dz_ik = g * ((double)P_ik / N);  m_k = (chunk rule over i of 1 * dz_ik) / N;
//                   q_k = (chunk rule over i of dz_ik * (double)z_ik) / (N - 1);
//                   dh_ik = (float)(((dz_ik - m_k) - ((double)z_ik * q_k) * ((sd_k + eps) / sd_k)) / (sd_k + eps)).
//                   With NO_STANDARDIZE dh = (float)dz.  dz is formed again wherever it is read; it is never stored.
//   zero variance   nothing is clamped.  sd_k = 0 with eps > 0: z = +0, a finite loss, and NaN in column k of dh alone (0 * 0 * inf);
//                   with eps = 0 that z is NaN (0 / 0, as in rlap_cca.h): the terms, column k of dh and the whole dh of the other view
//                   are NaN.
//
// The work map of the cross kernel.  The F columns are cut into nst = ceil(nft / 2) super tiles of 64 columns.  A workgroup of four
// waves takes a block row I and the four super-tile pairs (I, J0), ..., (I, J0 + 3), J0 a multiple of 4: it stages 32 rows x 64
// columns of z1 and 32 rows x 64 NW columns of z2, NW = cross_instance(nft).  Wave w owns pair (I, J0 + w) -- 2 x 2 accumulator
// tiles -- when J0 + w < nst.  All nst^2 pairs are computed, not a triangle.  Where nft is odd the second tile of the last super
// tile is clamped to the last tile: it is computed twice and stored once.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rlap_cca.h"
#include "rlap_spmm.h"
#include "rlap_tile32.h"

namespace rlap {
namespace bt {

using tile32::TILE;
using tile32::num_tiles;
using tile32::padded_rows;
using tile32::feature_tiles;
using tile32::padded_features;
using tile32::reg_row;

constexpr int MAX_F = cca::MAX_F;         // feature columns of a call
constexpr int SUPER = cca::SUPER;         // a wave owns SUPER x SUPER tiles: a 64 x 64 super-tile pair
constexpr int GROUP_PAIRS = 4;            // super-tile pairs of a workgroup (one per wave), all of one block row
constexpr int64_t TARGET_GROUPS = 256;    // workgroups the cross kernel aims at: what num_parts() is made from
constexpr int64_t MAX_PARTS = 64;         // (bounds the part accumulators of the arena)
constexpr int NO_STANDARDIZE = 1;         // flags bit 0
constexpr int FLAGS_MASK = NO_STANDARDIZE;

RLAP_SPMM_HD bool lambd_ok(double l) { return cca::lambd_ok(l); }
RLAP_SPMM_HD bool eps_ok(double e) { return cca::lambd_ok(e); }   // (finite and >= 0 too)
RLAP_SPMM_HD bool flags_ok(int flags) { return (flags & ~FLAGS_MASK) == 0; }

// ---- the work map
RLAP_SPMM_HD int super_tiles(int64_t F) { return cca::super_tiles(F); }
// the groups of four pairs of a block row, and the workgroups of a part: every block row has the same number
RLAP_SPMM_HD int row_groups(int64_t F) { return (super_tiles(F) + GROUP_PAIRS - 1) / GROUP_PAIRS; }
RLAP_SPMM_HD int pair_groups(int64_t F) { return super_tiles(F) * row_groups(F); }
// workgroup grp (0 <= grp < pair_groups) -> its block row I and its first block column J0
RLAP_SPMM_HD void group_of(int grp, int rgroups, int* I, int* J0) {
    *I = grp / rgroups;
    *J0 = (grp - *I * rgroups) * GROUP_PAIRS;
}
// whether wave w of the workgroup at J0 owns a pair
RLAP_SPMM_HD bool wave_active(int J0, int w, int nst) { return J0 + w < nst; }
// tile a (0 or 1) of super tile I, kept inside the nft tiles of the image
RLAP_SPMM_HD int tile_of(int I, int a, int nft) { return cca::tile_of(I, a, nft); }
// whether the wave of pair (I, J) stores its tile (a, b): inside the image.  (A clamped tile is not.)
RLAP_SPMM_HD bool tile_stored(int I, int J, int a, int b, int nft) { return SUPER * I + a < nft && SUPER * J + b < nft; }

// Which instances the launchers of rlap_bt.hip take for nft = feature_tiles(F); 0 for an nft outside [1, MAX_F / TILE].
//   k_bt_cross<NW>   the staged slab of z2 is 64 NW columns wide, NW = the pairs a workgroup can hold: 1, 2 or 4.
//   k_bt_zr<NCT>     rlap_cca.h's rule (zr_instance).
RLAP_SPMM_HD int cross_instance(int nft) {
    if (nft < 1 || nft > MAX_F / TILE) return 0;
    const int nst = (nft + SUPER - 1) / SUPER;
    return nst <= 1 ? 1 : (nst <= 2 ? 2 : GROUP_PAIRS);
}
RLAP_SPMM_HD int zr_instance(int nft) { return cca::zr_instance(nft); }

// The parts of the rows: a function of (N, F) alone, built as cca::num_parts from this kernel's own group count.
RLAP_SPMM_HD int64_t num_parts(int64_t N, int64_t F) {
    const int64_t T = num_tiles(N), G = pair_groups(F);
    if (T < 1 || G < 1) return 1;
    int64_t p = (TARGET_GROUPS + G - 1) / G;
    if (p > MAX_PARTS) p = MAX_PARTS;
    return p < 1 ? 1 : (p > T ? T : p);
}
RLAP_SPMM_HD int64_t part_begin(int64_t N, int64_t F, int64_t p) { return (p * num_tiles(N) / num_parts(N, F)) * TILE; }   // a ROW; (T < 2^26, p <= 64)

// ---- the values
RLAP_SPMM_HD double scale_of(double sd, double eps) { return sd + eps; }
RLAP_SPMM_HD float zval(float h, double mean, double scale) { return (float)(cca::centred(h, mean) / scale); }
RLAP_SPMM_HD float cross_step(float acc, float x, float y) { return cca::gram_step(acc, x, y); }
RLAP_SPMM_HD double c_of(double S, int64_t N) { return S / (double)N; }
RLAP_SPMM_HD double on_entry(double c) { return 1.0 - c; }                          // its square is the term
RLAP_SPMM_HD double off_entry(double c, bool diagonal) { return diagonal ? 0.0 : c; }   // its square is the term
RLAP_SPMM_HD double loss_of(double on, double lambd, double off) {
    const double u = lambd * off;
    return on + u;
}

RLAP_SPMM_HD float w_of(float cross, bool diagonal, double lambd) {
    if (diagonal) {
        const double d = 1.0 - (double)cross;
        return (float)(-2.0 * d);
    }
    const double l2 = 2.0 * lambd;
    return (float)(l2 * (double)cross);
}
RLAP_SPMM_HD double dz_of(double g, float P, int64_t N) {
    const double t = (double)P / (double)N;
    return g * t;
}
RLAP_SPMM_HD double col_m(double total, int64_t N) { return cca::col_m(total, N); }
RLAP_SPMM_HD double col_q(double total, int64_t N) { return cca::col_q(total, N); }
RLAP_SPMM_HD float dh_of(double dz, double m, float z, double q, double sd, double eps) {
    const double scale = scale_of(sd, eps);
    const double a = dz - m;
    const double b = (double)z * q;
    const double r = scale / sd;
    const double br = b * r;
    return (float)((a - br) / scale);
}

// the chunk rule over n terms c(e) * x(e)
template <class Coef, class Feat>
RLAP_SPMM_HD double rule_sum(int64_t n, Coef c, Feat x) { return cca::rule_sum(n, c, x); }

}  // namespace bt
}  // namespace rlap
