// rlap_linear.h -- the rule of the fused dense layer (rlap_linear_act / rlap_linear_act_backward, rlap_linear.hip):
// y = act(x W + b) and its gradients, every value and the order of every sum.  Plain __host__ __device__ functions without any HIP
// dependency, as rlap_bt.h: tests/csrc/linear_mirror.cc compiles this file with g++ (contraction off, as the library) and computes
// the same bits; tests/csrc/linear_main.cc runs the index arithmetic under the sanitizers; the kernels read the same functions.
// Where a value is rlap_cca.h's, rlap_tile32.h's or rlap_spmm.h's it is that function, not a copy of it.
//
// Inputs: x (M, Fin) float32 row-major, 1 <= M < 2^31 -- an (L, N, Fin) tensor is its M = L N rows, every layer shares the weight;
// W (Fin, Fout) float32 row-major, or with flags bit 0 (WEIGHT_OUT_IN) (Fout, Fin), torch.nn.Linear's layout; b (Fout,) float32 or
// absent; 1 <= Fin, Fout <= 512; act one of ACT_NONE, ACT_RELU, ACT_ELU; alpha (ELU's) finite and > 0.  "The chunk rule" is
// rlap_spmm.h's, as in rlap_cca.h.
//
//   forward     acc_io = the float32 fmaf chain over k = 0 .. padded_features(Fin) - 1 in increasing order from +0 of
//               fmaf(x_ik, W_ko, acc), the columns behind Fin as fmaf(0, 0, acc) -- what v_mfma_f32_32x32x2_f32 computes;
//               v = (double)acc_io + (double)b_o (v = (double)acc_io without a bias);
//               a = v (none);  a = v > 0 ? v : +0 (relu);  a = v > 0 ? v : alpha * expm1(v) (elu);  y_io = (float)a: one rounding.
//   backward    from stored float32 values only (x, W, y, gy).
//               d_io = 1 (none);  y_io > 0 ? 1 : 0 (relu);  y_io > 0 ? 1 : (double)y_io + alpha (elu);
//               t_io = (float)((double)gy_io * d_io): formed again wherever it is read, never stored as an (M, Fout) tensor.
//               gx_ik = the float32 fmaf chain over o = 0 .. padded_features(Fout) - 1 from +0 of fmaf(t_io, W_ko, acc).
//               gW_ko = (float)(0 + part 0 + part 1 + ... in float64), a part being the float32 fmaf chain over its rows i in
//               increasing order from +0 of fmaf(x_ik, t_io, acc).  The parts are the row ranges
//               [part_begin(M, Fin, Fout, p), part_begin(M, Fin, Fout, p + 1)), multiples of 32 rows, a function of
//               (M, Fin, Fout) alone; a row >= M takes its turn as fmaf(0, 0, acc).
//               gb_o = (float)(the chunk rule over i of 1 * (double)t_io).
//
// The work maps.
//   product     (forward and input gradient: (M, K) x (K, C) -> (M, C) with nct = feature_tiles(C) column tiles.)  A workgroup of
//               four waves takes row_tiles(nct) consecutive 32-row tiles and all nct column tiles: wave w works on row tile
//               w / col_waves(nct) of the workgroup's and owns the column tiles w % col_waves + col_waves j, j = 0 .. NCT - 1,
//               NCT = product_instance(nct) the kernel's instance.  col_waves is 1, 2, 4 for nct = 1, 2, >= 3: at narrow outputs
//               the waves that would idle take further rows instead.
//   weight grad the Fin columns are cut into super tiles of 64, and so are the Fout columns.  A workgroup takes (part, super tile I
//               of Fin, group of four super tiles J0 .. J0 + 3 of Fout); wave w owns the pair (I, J0 + w), 2 x 2 accumulator tiles,
//               when J0 + w < super_tiles(Fout).  Where a tile count is odd the second tile of the last super tile is clamped to
//               the last tile: computed twice, stored once.  NW = cross_instance(Fout) pairs fit the staged slab of t.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rlap_cca.h"
#include "rlap_spmm.h"
#include "rlap_tile32.h"

namespace rlap {
namespace linear {

using tile32::TILE;
using tile32::num_tiles;
using tile32::padded_rows;
using tile32::feature_tiles;
using tile32::padded_features;
using tile32::reg_row;

constexpr int MAX_F = cca::MAX_F;         // columns of x and of y, at most
constexpr int SUPER = cca::SUPER;         // the weight gradient's waves own SUPER x SUPER tiles
constexpr int GROUP_PAIRS = 4;            // super-tile pairs of a workgroup of the weight gradient (one per wave)
constexpr int WAVES = 4;                  // waves of a workgroup of either kernel
constexpr int64_t TARGET_GROUPS = 1024;   // workgroups the weight gradient aims at (four a CU): what num_parts() is made from
constexpr int64_t MAX_PARTS = 1024;       // (bounds the part accumulators of the arena: 64 MiB at the most)
constexpr int WEIGHT_OUT_IN = 1;          // flags bit 0: W is (Fout, Fin)
constexpr int FLAGS_MASK = WEIGHT_OUT_IN;
enum { ACT_NONE = 0, ACT_RELU = 1, ACT_ELU = 2 };

// ---- the argument checks
RLAP_SPMM_HD bool flags_ok(int flags) { return (flags & ~FLAGS_MASK) == 0; }
RLAP_SPMM_HD bool act_ok(int act) { return act == ACT_NONE || act == ACT_RELU || act == ACT_ELU; }
RLAP_SPMM_HD bool alpha_ok(double a) { return a > 0.0 && a <= 1.7976931348623157e308; }   // (false for a NaN and for inf)
RLAP_SPMM_HD bool features_ok(int64_t F) { return F >= 1 && F <= MAX_F; }
RLAP_SPMM_HD bool rows_ok(int64_t M) { return M >= 1 && M < ((int64_t)1 << 31); }
// whether rows of F floats from a base address can be read 16 bytes at a time: the lane path, a function of the shape and the
// base pointers' alignment alone (both paths give the same bits)
RLAP_SPMM_HD bool vec_ok(int64_t F, uint64_t address_bits) { return F % 4 == 0 && (address_bits & 15) == 0; }

// element (k, o) of the weight in either layout
RLAP_SPMM_HD int64_t weight_index(int64_t k, int64_t o, int64_t Fin, int64_t Fout, int flags) {
    return (flags & WEIGHT_OUT_IN) ? o * Fin + k : k * Fout + o;
}

// ---- the work map of the product kernels
RLAP_SPMM_HD int col_waves(int nct) { return nct <= 1 ? 1 : (nct <= 2 ? 2 : WAVES); }
RLAP_SPMM_HD int row_tiles(int nct) { return WAVES / col_waves(nct); }
// column tiles a wave holds: the instance of the kernel; 0 for an nct outside [1, MAX_F / TILE]
RLAP_SPMM_HD int product_instance(int nct) {
    if (nct < 1 || nct > MAX_F / TILE) return 0;
    return (nct + col_waves(nct) - 1) / col_waves(nct);
}
RLAP_SPMM_HD int64_t product_groups(int64_t M, int nct) { return (num_tiles(M) + row_tiles(nct) - 1) / row_tiles(nct); }
// wave w of workgroup g -> its row tile (may lie behind the last: then the wave only helps to stage) and its j-th column tile
// (owned when < nct)
RLAP_SPMM_HD int64_t wave_row_tile(int64_t g, int w, int nct) { return g * row_tiles(nct) + w / col_waves(nct); }
RLAP_SPMM_HD int wave_col_tile(int w, int j, int nct) { return w % col_waves(nct) + col_waves(nct) * j; }

// ---- the work map of the weight gradient
RLAP_SPMM_HD int super_tiles(int64_t F) { return cca::super_tiles(F); }
RLAP_SPMM_HD int row_groups(int64_t Fout) { return (super_tiles(Fout) + GROUP_PAIRS - 1) / GROUP_PAIRS; }
RLAP_SPMM_HD int pair_groups(int64_t Fin, int64_t Fout) { return super_tiles(Fin) * row_groups(Fout); }
RLAP_SPMM_HD void group_of(int grp, int rgroups, int* I, int* J0) {
    *I = grp / rgroups;
    *J0 = (grp - *I * rgroups) * GROUP_PAIRS;
}
RLAP_SPMM_HD bool wave_active(int J0, int w, int nst_out) { return J0 + w < nst_out; }
RLAP_SPMM_HD int tile_of(int I, int a, int nft) { return cca::tile_of(I, a, nft); }
RLAP_SPMM_HD bool tile_stored(int I, int J, int a, int b, int nft_in, int nft_out) { return SUPER * I + a < nft_in && SUPER * J + b < nft_out; }
// super tiles of t a workgroup stages: 1, 2 or 4; 0 for a tile count outside [1, MAX_F / TILE]
RLAP_SPMM_HD int cross_instance(int nft_out) {
    if (nft_out < 1 || nft_out > MAX_F / TILE) return 0;
    const int nst = (nft_out + SUPER - 1) / SUPER;
    return nst <= 1 ? 1 : (nst <= 2 ? 2 : GROUP_PAIRS);
}
// the parts of the rows: a function of (M, Fin, Fout) alone
RLAP_SPMM_HD int64_t num_parts(int64_t M, int64_t Fin, int64_t Fout) {
    const int64_t T = num_tiles(M), G = pair_groups(Fin, Fout);
    if (T < 1 || G < 1) return 1;
    int64_t p = (TARGET_GROUPS + G - 1) / G;
    if (p > MAX_PARTS) p = MAX_PARTS;
    return p < 1 ? 1 : (p > T ? T : p);
}
RLAP_SPMM_HD int64_t part_begin(int64_t M, int64_t Fin, int64_t Fout, int64_t p) {   // a ROW; (T < 2^26, p <= 1024)
    return (p * num_tiles(M) / num_parts(M, Fin, Fout)) * TILE;
}

// ---- the values
RLAP_SPMM_HD float chain_step(float acc, float x, float y) { return cca::gram_step(acc, x, y); }
RLAP_SPMM_HD float y_of(float acc, bool has_bias, float b, int act, double alpha) {
    double v = (double)acc;
    if (has_bias) v = v + (double)b;
    double a = v;
    if (act == ACT_RELU) a = v > 0.0 ? v : 0.0;
    else if (act == ACT_ELU) a = v > 0.0 ? v : alpha * expm1(v);
    return (float)a;
}
RLAP_SPMM_HD double d_of(float y, int act, double alpha) {
    if (act == ACT_RELU) return y > 0.0f ? 1.0 : 0.0;
    if (act == ACT_ELU) return y > 0.0f ? 1.0 : (double)y + alpha;
    return 1.0;
}
RLAP_SPMM_HD float t_of(float gy, float y, int act, double alpha) { return (float)((double)gy * d_of(y, act, alpha)); }

// the chunk rule over n terms c(e) * x(e)
template <class Coef, class Feat>
RLAP_SPMM_HD double rule_sum(int64_t n, Coef c, Feat x) { return cca::rule_sum(n, c, x); }

}  // namespace linear
}  // namespace rlap
