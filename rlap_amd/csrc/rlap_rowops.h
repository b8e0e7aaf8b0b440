// rlap_rowops.h -- the rule of the fused bias, activation and dropout pass (rlap_bias_act_dropout / _backward, rlap_rowops.hip,
// DESIGN 4.28): every value of both calls, the dropout coin, the order of every sum and the size of the arena.  Plain
// __host__ __device__ functions without any HIP dependency, as rlap_norm.h: tests/csrc/rowops_mirror.cc compiles this file with g++
// (contraction off, as the library) and computes the same bits; tests/csrc/rowops_main.cc runs the map under the sanitizers; the
// kernels read the same functions.
//
// x is (L, N, F) float32; element (l, i, k) is row i, column k of layer l; every statement is float64 and rounded on its own.
//
//   coin       T = (uint32)llrint(p * 65536), at most 65535;  one 64-bit word serves the four columns 4q .. 4q + 3 of a row:
//              word(l, i, q) = mix64(mix64((seed + l) ^ COIN_SALT) ^ mix64(i * ceil(F / 4) + q)),  bits(k) = (word >> 16 (k % 4)) & 65535;
//              element (l, i, k) is kept iff bits >= T;  s = 1 / (1 - T / 65536), so that the expectation is exact for the
//              probability T / 65536 that is used.  The coin depends on (seed, l, i, k, F, T) alone -- not on the launch, the lane
//              path or L --, and layer l of a call is layer 0 of the call with seed + l (the project's convention for views).
//              COIN_SALT is this call's own: the coin is not the one of rlap_edge_drop under the same seed.  Without
//              RLAP_ROW_TRAINING, or with T = 0, no coin is drawn: every element is kept and s = 1, which multiplies exactly --
//              the bits of the call without dropout.
//   forward    v = (double)x + (double)b (b = 0 without a bias);  a = act(v): none, relu (v > 0 ? v : +0) or prelu (v > 0 ? v :
//              slope * v), the slope one value or one a column;  y = (float)(keep ? a * s : +0).
//   backward   t = (double)gy * s;  gv = keep ? t * act'(v) : +0 (relu: v > 0 ? 1 : 0; prelu: v > 0 ? 1 : slope);  gx = (float)gv;
//              A = the chunk rule (rlap_spmm.h) of 1 * gv over the rows of a column;  gbias = (float)(0 + A of layer 0 + A of layer
//              1 + ...);  C = the chunk rule of 1 * c_i, c_i = t * v where the element is kept and v <= 0, else +0;  gslope per
//              channel = (float)(0 + C of layer 0 + ...), the single slope (float)(0 + that float64 sum of column 0 + of column
//              1 + ...), as rlap_norm.h defines its C.
// Nothing is kept between the calls: the backward call draws the forward call's coins again from (seed, p).
#pragma once
#include <math.h>
#include <stdint.h>

#include "rlap_core.h"
#include "rlap_norm.h"

namespace rlap {
namespace rowops {

constexpr int MAX_F = norm::MAX_F;
// the flags of include/rlap_hip.h (RLAP_ROW_*)
constexpr int ACT_RELU = 1, ACT_PRELU = 2, SLOPE_PER_CHANNEL = 4, TRAINING = 8;
constexpr int ALL_FLAGS = 15;
constexpr uint64_t COIN_SALT = 0x726F776F7073646Full;   // "rowopsdo"

RLAP_SPMM_HD bool p_ok(double p) { return p >= 0.0 && p < 1.0; }   // (false for a NaN)
// what both exports refuse before anything is launched
RLAP_SPMM_HD bool args_ok(int64_t L, int64_t N, int64_t F, int flags, bool has_slope, double p) {
    if (flags & ~ALL_FLAGS) return false;
    if ((flags & ACT_RELU) && (flags & ACT_PRELU)) return false;
    if ((flags & ACT_PRELU) && !has_slope) return false;
    if ((flags & SLOPE_PER_CHANNEL) && !(flags & ACT_PRELU)) return false;
    if (L < 1 || N < 1 || F < 1 || F > MAX_F) return false;
    return p_ok(p);
}

// ---- the coin
RLAP_SPMM_HD uint32_t threshold(double p, int flags) {
    if (!(flags & TRAINING)) return 0;
    const long long t = llrint(p * 65536.0);
    return t > 65535 ? 65535u : (uint32_t)t;
}
RLAP_SPMM_HD double scale(uint32_t T) { return 1.0 / (1.0 - (double)T / 65536.0); }
RLAP_SPMM_HD int64_t quads(int64_t F) { return (F + 3) >> 2; }
RLAP_SPMM_HD uint64_t coin_layer(uint64_t seed, int64_t l) { return mix64((seed + (uint64_t)l) ^ COIN_SALT); }
RLAP_SPMM_HD uint64_t coin_word(uint64_t layer, int64_t i, int64_t q, int64_t F) { return mix64(layer ^ mix64((uint64_t)(i * quads(F) + q))); }
RLAP_SPMM_HD uint32_t coin_bits(uint64_t word, int64_t k) { return (uint32_t)(word >> (16 * (int)(k & 3))) & 65535u; }
RLAP_SPMM_HD bool keeps(uint32_t bits, uint32_t T) { return bits >= T; }
RLAP_SPMM_HD bool keep_of(uint64_t seed, int64_t l, int64_t i, int64_t k, int64_t F, uint32_t T) {
    return T == 0 || keeps(coin_bits(coin_word(coin_layer(seed, l), i, k >> 2, F), k), T);
}

// ---- the values.  Col is what a column's elements share: the bias and the slope.
struct Col { double b, a; };
RLAP_SPMM_HD double act(double v, int flags, double a) {
    if (flags & ACT_RELU) return v > 0.0 ? v : 0.0;
    if (flags & ACT_PRELU) return v > 0.0 ? v : a * v;
    return v;
}
RLAP_SPMM_HD double act_grad(double v, int flags, double a) {
    if (flags & ACT_RELU) return v > 0.0 ? 1.0 : 0.0;
    if (flags & ACT_PRELU) return v > 0.0 ? 1.0 : a;
    return 1.0;
}
RLAP_SPMM_HD double v_of(float x, const Col& c) { return (double)x + c.b; }
RLAP_SPMM_HD float y_of(float x, const Col& c, bool keep, double s, int flags) {
    const double a = act(v_of(x, c), flags, c.a);
    return (float)(keep ? a * s : 0.0);
}
RLAP_SPMM_HD double gv_of(float x, float gy, const Col& c, bool keep, double s, int flags) {
    const double t = (double)gy * s;
    return keep ? t * act_grad(v_of(x, c), flags, c.a) : 0.0;
}
RLAP_SPMM_HD double slope_term(float x, float gy, const Col& c, bool keep, double s) {
    const double v = v_of(x, c);
    const double t = (double)gy * s;
    return keep && v <= 0.0 ? t * v : 0.0;
}

// ---- the work map is rlap_norm.h's: lanes along the columns, 16 bytes a lane where F and the pointers allow (norm::dispatch), rows
// narrower than a wave sharing it, one item per (layer, group of chunks, column tile) (norm::item_of).  The forward pass and a
// backward pass without parameter gradients have no order to keep and cut their items into row ranges (norm::apply_split); a
// backward pass that leaves chunk sums keeps a chunk's rows with one lane, in row order.
RLAP_SPMM_HD int split_of(int64_t items, bool sums) { return sums ? 0 : norm::apply_split(items); }

// ---- the arena of the backward call: nothing without parameter gradients; else `planes` planes of chunk sums (L, chunks, F) --
// A, and C where the slope's gradient is asked for --, then their per-layer totals (planes, L, F); float64, each piece on a
// 256-byte boundary.  The forward call takes none.
RLAP_SPMM_HD int planes_of(bool want_bias, bool want_slope) { return want_slope ? 2 : (want_bias ? 1 : 0); }
RLAP_SPMM_HD int64_t backward_bytes(int64_t L, int64_t N, int64_t F, int planes) {
    return planes ? norm::piece(norm::part_doubles(L, N, F, planes)) + norm::piece((int64_t)planes * L * F) : 0;
}

// ---- layer norm (rlap_layer_norm / _backward): per row of F columns, float64.
//   row sum    the order depends on F alone: lane t of 64 owns the columns 256 m + 4 t + v (v < 4, m = 0, 1, ...: 16 bytes a lane and
//              step) and adds its terms from 0 in ascending (m, v); the 64 partials meet in an xor butterfly over 32, 16, 8, 4, 2, 1
//              lanes (row_sum).  A lane without a column holds +0, so a row of few columns may run the butterfly's last steps alone.
//   forward    mean = row sum of x / F;  d = x - mean;  var = row sum of d * d / F (biased, as torch.nn.LayerNorm; a second pass over
//              the row, which sits in registers);  rstd = 1 / sqrt(var + eps) (a constant row: 1 / sqrt(eps), no NaN);  xh = d * rstd;
//              v = xh * w + b (two rounded operations; w = 1, b = 0 without them);  a = act(v);  y = (float)(keep ? a * s : +0), the
//              coin as above.
//   backward   gv = keep ? ((double)gy * s) * act'(v) : +0;  g = gv * w;  mg = row sum of g / F;  mgx = row sum of g * xh / F;
//              gx = (float)(rstd * ((g - mg) - xh * mgx));  gweight = the chunk rule over the rows of gv * xh, gbias of 1 * gv, gslope
//              of the slope terms (kept, v <= 0: ((double)gy * s) * v), the layers then added in order, the single slope then over
//              the columns in order -- as above.
// Nothing but x is kept for the backward call: mean and rstd are formed again from the row.
RLAP_SPMM_HD bool ln_args_ok(int64_t L, int64_t N, int64_t F, int flags, bool has_slope, double p, double eps) {
    return args_ok(L, N, F, flags, has_slope, p) && norm::eps_ok(eps);
}
RLAP_SPMM_HD int ln_steps(int64_t F) { return (int)((F + 255) >> 8); }
RLAP_SPMM_HD int64_t ln_column(int t, int m, int v) { return 256 * (int64_t)m + 4 * t + v; }
// lanes of a row: 2^lg >= ceil(F / 4), at most 64; the rows of a wave: 64 >> lg
RLAP_SPMM_HD int ln_lg(int64_t F) { int lg = 0; while (lg < 6 && ((int64_t)4 << lg) < F) ++lg; return lg; }
// the row kernel's instance: the 16-byte steps of a lane, ceil(F / 256) rounded up to a power of two -- 1, 2 and 4 are template
// instances that hold the row in registers, 8 and 16 the kernel that parks it in LDS
RLAP_SPMM_HD int ln_instance(int64_t F) { int m = 1; while (m < ln_steps(F)) m <<= 1; return m; }
template <class Term>
RLAP_SPMM_HD double row_sum(int64_t F, Term term) {
    double part[64];
    for (int t = 0; t < 64; ++t) {
        double acc = 0.0;
        for (int m = 0; m < ln_steps(F); ++m)
            for (int v = 0; v < 4; ++v) {
                const int64_t k = ln_column(t, m, v);
                if (k < F) acc = acc + term(k);
            }
        part[t] = acc;
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int j = 0; j < 64; ++j)
            if (!(j & off)) { const double s = part[j] + part[j ^ off]; part[j] = s; part[j ^ off] = s; }
    return part[0];
}
RLAP_SPMM_HD double ln_mean(double sum, int64_t F) { return sum / (double)F; }
RLAP_SPMM_HD double ln_rstd(double var, double eps) { return 1.0 / sqrt(var + eps); }
struct Row { double mean, rstd; };
struct LnCol { double w, b, a; };
RLAP_SPMM_HD double ln_centred(float x, double mean) { return (double)x - mean; }
RLAP_SPMM_HD double ln_square(double d) { return d * d; }
RLAP_SPMM_HD double ln_xhat(float x, const Row& r) { return ln_centred(x, r.mean) * r.rstd; }
RLAP_SPMM_HD double ln_affine(double xh, const LnCol& c) { const double t = xh * c.w; return t + c.b; }
RLAP_SPMM_HD float ln_y(float x, const Row& r, const LnCol& c, bool keep, double s, int flags) {
    const double a = act(ln_affine(ln_xhat(x, r), c), flags, c.a);
    return (float)(keep ? a * s : 0.0);
}
RLAP_SPMM_HD double ln_gv(float x, float gy, const Row& r, const LnCol& c, bool keep, double s, int flags) {
    const double t = (double)gy * s;
    return keep ? t * act_grad(ln_affine(ln_xhat(x, r), c), flags, c.a) : 0.0;
}
RLAP_SPMM_HD double ln_g(double gv, const LnCol& c) { return gv * c.w; }
RLAP_SPMM_HD double ln_gxh(double g, double xh) { return g * xh; }
RLAP_SPMM_HD float ln_gx(double g, double xh, double mg, double mgx, double rstd) {
    const double p = g - mg;
    const double q = xh * mgx;
    return (float)(rstd * (p - q));
}
RLAP_SPMM_HD double ln_slope_term(float x, float gy, const Row& r, const LnCol& c, bool keep, double s) {
    const double v = ln_affine(ln_xhat(x, r), c);
    const double t = (double)gy * s;
    return keep && v <= 0.0 ? t * v : 0.0;
}
// the arena of the backward call: nothing without parameter gradients; else the rows' (mean, rstd) (L, N, 2), `planes` planes of
// chunk sums -- A, gweight's, and C where the slope's gradient is asked for -- and their per-layer totals
RLAP_SPMM_HD int ln_planes_of(bool want_weight, bool want_bias, bool want_slope) { return want_slope ? 3 : ((want_weight || want_bias) ? 2 : 0); }
RLAP_SPMM_HD int64_t ln_backward_bytes(int64_t L, int64_t N, int64_t F, int planes) {
    return planes ? backward_bytes(L, N, F, planes) + norm::piece(2 * L * N) : 0;
}

}  // namespace rowops
}  // namespace rlap
