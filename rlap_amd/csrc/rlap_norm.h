// rlap_norm.h -- the rule of the per-view batch norm with fused activations (rlap_batch_norm / rlap_batch_norm_backward,
// rlap_norm.hip): every value of the call, the order of every sum, and the arithmetic that maps the work of a call to
// (layer, chunk, column tile).  Plain __host__ __device__ functions without any HIP dependency, as rlap_cca.h:
// tests/csrc/norm_mirror.cc compiles this file with g++ (contraction off, as the library) and computes the same bits;
// tests/csrc/norm_main.cc runs the map functions under the sanitizers; the kernels read the same functions.
//
// x is (L, N, F) float32; every statement is per layer l and column k, in float64.  "The chunk rule" is rlap_spmm.h's: the terms
// c_e * x_e of a list (product rounded, add rounded) summed from 0 in chunks of 256 in order, the chunk sums added to 0 in order.
//
//   training forward   u_i = pre(x_i) (relu: x > 0 ? x : +0);  c = u_0;  d_i = u_i - c;  s1 = chunk rule of 1 * d_i;  s2 = chunk rule
//                      of d_i * d_i;  m = s1 / N;  var = s2 / N - m * m, 0 when negative;  rstd = 1 / sqrt(var + eps);  mean = c + m;
//                      xh_i = (d_i - m) * rstd;  v_i = xh_i * w + b (two rounded operations; w = 1, b = 0 without them);
//                      y_i = (float)post(v_i) (relu: v > 0 ? v : +0; prelu: v > 0 ? v : a * v).  A column of zero variance has
//                      rstd = 1 / sqrt(eps).  One pass over x serves both sums, and the shift c keeps s2 / N - m * m from cancelling.
//   running buffers    float32, the layers in order l = 0 .. L-1, each step rounded as torch stores it:
//                      rm = (float)((1 - momentum) * rm + momentum * mean);  rv the same with var * N / (N - 1).
//   evaluation         xh_i = (u_i - (double)rm) * rstd with rstd = 1 / sqrt((double)rv + eps); no sums, no buffer written.
//   backward           gv_i = (double)gy_i * post'(v_i) (relu: v > 0 ? 1 : 0; prelu: v > 0 ? 1 : a);  A = chunk rule of 1 * gv_i;
//                      B = chunk rule of gv_i * xh_i;  gu_i = (rstd * w) * ((gv_i - A / N) - xh_i * (B / N)), in evaluation mode
//                      (rstd * w) * gv_i;  gx_i = (float)(pre'(x_i) * gu_i) (relu: x > 0).  gbias = (float)(0 + A of layer 0 + A of
//                      layer 1 + ...), gweight the same over B.  C = chunk rule of 1 * t_i, t_i = (double)gy_i * v_i where v_i <= 0,
//                      else +0;  gslope per channel = (float)(0 + C of layer 0 + ...), the single slope (float)(0 + that float64 sum of
//                      column 0 + of column 1 + ...).
// u, xh and v are functions of x and of three float64 values a column (c, m, rstd: the call's `stat`); they are formed again
// wherever they are read and never stored.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rlap_readout.h"
#include "rlap_spmm.h"

namespace rlap {
namespace norm {

constexpr int MAX_F = 4096;   // feature columns of a call (project_dim = hidden_dim * num_layers of the graph-level encoder)
// the flags of include/rlap_hip.h (RLAP_NORM_*)
constexpr int PRE_RELU = 1, POST_RELU = 2, POST_PRELU = 4, SLOPE_PER_CHANNEL = 8, EVAL = 16;
constexpr int ALL_FLAGS = 31;

RLAP_SPMM_HD bool eps_ok(double e) { return e > 0.0 && e <= 1.7976931348623157e308; }          // (false for a NaN and for inf)
RLAP_SPMM_HD bool momentum_ok(double m) { return m >= 0.0 && m <= 1.0; }                       // (false for a NaN)
// what both exports refuse before anything is launched
RLAP_SPMM_HD bool args_ok(int64_t L, int64_t N, int64_t F, int flags, bool has_slope, bool has_running, double eps, double momentum) {
    if (flags & ~ALL_FLAGS) return false;
    if ((flags & POST_RELU) && (flags & POST_PRELU)) return false;
    if ((flags & POST_PRELU) && !has_slope) return false;
    if ((flags & EVAL) && !has_running) return false;
    if (L < 1 || F < 1 || F > MAX_F || N < ((flags & EVAL) ? 1 : 2)) return false;
    return eps_ok(eps) && momentum_ok(momentum);
}

// ---- the values
RLAP_SPMM_HD double pre(float x, int flags) { return (flags & PRE_RELU) ? (x > 0.0f ? (double)x : 0.0) : (double)x; }
RLAP_SPMM_HD double pre_grad(float x, int flags) { return (flags & PRE_RELU) ? (x > 0.0f ? 1.0 : 0.0) : 1.0; }
RLAP_SPMM_HD double post(double v, int flags, double a) {
    if (flags & POST_RELU) return v > 0.0 ? v : 0.0;
    if (flags & POST_PRELU) return v > 0.0 ? v : a * v;
    return v;
}
RLAP_SPMM_HD double post_grad(double v, int flags, double a) {
    if (flags & POST_RELU) return v > 0.0 ? 1.0 : 0.0;
    if (flags & POST_PRELU) return v > 0.0 ? 1.0 : a;
    return 1.0;
}

RLAP_SPMM_HD double col_m(double s1, int64_t N) { return s1 / (double)N; }
RLAP_SPMM_HD double col_var(double s2, double m, int64_t N) {
    const double t = s2 / (double)N;
    const double mm = m * m;
    const double v = t - mm;
    return v < 0.0 ? 0.0 : v;   // (a NaN stays one)
}
RLAP_SPMM_HD double col_rstd(double var, double eps) { return 1.0 / sqrt(var + eps); }
RLAP_SPMM_HD double col_mean(double c, double m) { return c + m; }
RLAP_SPMM_HD double unbiased(double var, int64_t N) { const double t = var * (double)N; return t / (double)(N - 1); }
RLAP_SPMM_HD float running(float r, double momentum, double value) {
    const double keep = (1.0 - momentum) * (double)r;
    const double take = momentum * value;
    return (float)(keep + take);
}

// what a column's elements share: training c = u_0, m, rstd; evaluation c = (double)running_mean, m unused, rstd from running_var
struct Col { double c, m, rstd, w, b, a; };
RLAP_SPMM_HD double xhat(double u, const Col& k, int flags) {
    const double d = u - k.c;
    return (flags & EVAL) ? d * k.rstd : (d - k.m) * k.rstd;
}
RLAP_SPMM_HD double affine(double xh, const Col& k) { const double t = xh * k.w; return t + k.b; }
RLAP_SPMM_HD float y_of(float x, const Col& k, int flags) { return (float)post(affine(xhat(pre(x, flags), k, flags), k), flags, k.a); }

RLAP_SPMM_HD double gv_of(float gy, double v, const Col& k, int flags) { return (double)gy * post_grad(v, flags, k.a); }
RLAP_SPMM_HD double slope_term(float gy, double v) { return v <= 0.0 ? (double)gy * v : 0.0; }
// An = A / N and Bn = B / N (unused in evaluation mode)
RLAP_SPMM_HD float gx_of(float x, float gy, const Col& k, double An, double Bn, int flags) {
    const double xh = xhat(pre(x, flags), k, flags);
    const double gv = gv_of(gy, affine(xh, k), k, flags);
    const double sw = k.rstd * k.w;
    double gu;
    if (flags & EVAL) {
        gu = sw * gv;
    } else {
        const double p = gv - An;
        const double q = xh * Bn;
        gu = sw * (p - q);
    }
    return (float)(pre_grad(x, flags) * gu);
}

// ---- the work map.  Lanes run along the columns, 16 bytes (four columns) a lane where F and the pointers allow, else one column a
// lane: readout::dispatch for float32.  A row that takes P = 2^lg < 64 lanes shares its wave with the rows of C = 64 / P consecutive
// chunks; a wider row takes `ftiles` tiles of 64 lanes.  Work item w of a pass is (layer, group of C chunks, column tile); lane
// `lane` of it owns chunk q and the columns [f0, f0 + V).
RLAP_SPMM_HD readout::Dispatch dispatch(int64_t F, bool aligned16) { return readout::dispatch(F, 4, aligned16); }
RLAP_SPMM_HD int64_t chunk_groups(int64_t N, int lg) { const int64_t C = 64 >> lg; return (spmm::num_chunks(N) + C - 1) / C; }
RLAP_SPMM_HD int64_t num_items(int64_t L, int64_t N, const readout::Dispatch& d) { return L * chunk_groups(N, d.lg) * d.ftiles; }
constexpr int GROUP_WAVES = 4;         // waves of a workgroup of the passes
constexpr int64_t MAX_GRID = 2048;     // workgroups of a launch: a pass of more than MAX_GRID * GROUP_WAVES items strides over them
struct Item { int64_t l, q, f0, r0, r1; };   // rows [r0, r1) of layer l, columns [f0, f0 + V)
RLAP_SPMM_HD bool item_of(int64_t w, int lane, int64_t L, int64_t N, int64_t F, const readout::Dispatch& d, Item* it) {
    const int64_t groups = chunk_groups(N, d.lg), V = d.vec ? 4 : 1;
    if (w < 0 || w >= L * groups * d.ftiles || lane < 0 || lane > 63) return false;
    const int64_t lq = w / d.ftiles, ft = w - lq * d.ftiles;
    it->l = lq / groups;
    const int64_t qg = lq - it->l * groups;
    it->q = (qg << (6 - d.lg)) + (lane >> d.lg);
    it->f0 = (ft * 64 + (lane & ((1 << d.lg) - 1))) * V;
    if (it->f0 >= F || it->q >= spmm::num_chunks(N)) return false;
    it->r0 = spmm::chunk_begin(it->q);
    it->r1 = spmm::chunk_end(N, it->q);
    return true;
}

// The apply passes have no order to keep, so a pass of few items cuts each into 2^s ranges of CHUNK >> s rows, s <= 4, until it has
// APPLY_WAVES of them: part p of an item is rows [*r0, *r1), empty behind the chunk's end.
constexpr int64_t APPLY_WAVES = 4096;
RLAP_SPMM_HD int apply_split(int64_t items) { int s = 0; while (s < 4 && (items << s) < APPLY_WAVES) ++s; return s; }
RLAP_SPMM_HD void split_rows(const Item& it, int s, int64_t p, int64_t* r0, int64_t* r1) {
    const int64_t rb = spmm::CHUNK >> s;
    *r0 = it.r0 + p * rb;
    *r1 = *r0 + rb < it.r1 ? *r0 + rb : it.r1;
}

// ---- the arena: float64 pieces, each on a 256-byte boundary.  `sums` planes of chunk sums (L, chunks, F) -- s1, s2 forward;
// A, B and (PReLU) C backward --, then (2, L, F): forward the mean and the unbiased variance, backward A / N and B / N; backward also
// the totals A, B, C (3, L, F).
RLAP_SPMM_HD int64_t piece(int64_t doubles) { return (doubles * 8 + 255) & ~(int64_t)255; }
RLAP_SPMM_HD int backward_sums(int flags) { return (flags & POST_PRELU) ? 3 : 2; }
RLAP_SPMM_HD int64_t part_doubles(int64_t L, int64_t N, int64_t F, int sums) { return sums * L * spmm::num_chunks(N) * F; }
RLAP_SPMM_HD int64_t forward_bytes(int64_t L, int64_t N, int64_t F, int flags) {
    return (flags & EVAL) ? 0 : piece(part_doubles(L, N, F, 2)) + piece(2 * L * F);
}
RLAP_SPMM_HD int64_t backward_bytes(int64_t L, int64_t N, int64_t F, int flags) {
    return piece(part_doubles(L, N, F, backward_sums(flags))) + piece(2 * L * F) + piece(3 * L * F);
}

}  // namespace norm
}  // namespace rlap
