// rlap_g2l.h -- the rule of the fused graph-to-local losses (rlap_g2l_jsd / rlap_g2l_bootstrap and their backward calls, rlap_g2l.hip,
// DESIGN 4.17): every value of the calls and the order of every sum.  Plain __host__ __device__ functions without any HIP
// dependency, as rlap_infonce.h: tests/csrc/g2l_mirror.cc compiles this file with g++ (contraction off, as the library) and computes
// the same bits; tests/csrc/g2l_main.cc runs the index arithmetic under the sanitizers; the kernels read the same functions.
//
// Inputs: h (N, F) float32 node embeddings, g (G, F) float32 graph summaries, node_ptr [G+1]: node i belongs to graph g(i), the last
// graph j with node_ptr[j] <= i (empty graphs are stepped over; G > N is legal); for one graph, neg (N, F), the embeddings of the
// corrupted input.
//
//   score           s_ij = the float32 fmaf chain over k = 0 .. F-1 in increasing k from +0: acc = fmaf(g_jk, h_ik, acc) -- what
//                   v_mfma_f32_32x32x2_f32 computes.  Zero columns behind F add fmaf(0, 0, x).  JSD runs on the raw values, the
//                   bootstrap on the hat values of rlap_infonce.h (float64 norm, max(., 1e-12), one rounding).
//   JSD terms       m = min(|s|, 64) (a comparison that is false for a NaN: a score that is not finite gives m = 64, so the
//                   (int32_t) conversion inside expw never sees a NaN or an infinity);  e = expw(-m) in float32;
//                   relu(x) = x < 0 ? 0 : x in float64 (a NaN fails the comparison and stays);  softplus(+-s) = relu(+-s) +
//                   log1p((double)e).  A term is softplus -+ ln 2, and log1p(e) - ln 2 = log((1 + e) / 2) is taken in one piece:
//                   v = log1p(((double)e - 1) * 0.5), the float64 library function -- the one operation whose bits may differ
//                   between host and device.  Subtracting a rounded ln 2 from log1p(e) would leave an ABSOLUTE error of 1.1e-16
//                   in a term that is s / 2 near s = 0; v is accurate relative to itself, and a score of 0 gives exactly 0.
//                   nf = s - s in float32: +0 for a finite score, NaN for a NaN or an infinity;
//                   pos term = ln 2 - softplus(-s) = -(relu(-s) + v) + nf;   neg term = softplus(s) - ln 2 = (relu(s) + v) + nf.
//                   So a NaN score reaches its term through relu and through nf, an infinite one through nf: the loss is then NaN.
//                   Unlike torch's softplus there is no switch to the identity above 20 (the difference at 21 is 7.6e-10).
//   row sums        pos_i = the pos term of s_{i, g(i)}.
//                   G >= 2: neg_i over the 32-graph tiles t = 0 .. ceil(G / 32) - 1 in increasing order.  Two float64 sums run from
//                   0, one per lane half hf: half hf adds the neg terms of the graphs j = 32 t + reg_row(r, hf), r = 0 .. 15 in
//                   order, tile after tile; the graphs j >= G and j = g(i) are LEFT OUT, not added as zeros.  neg_i = half 0 +
//                   half 1.  The order depends on G alone.
//                   G == 1: neg_i = the neg term of s'_i = the chain of <neg_i, g_0>.
//   loss            E_pos = (sum of pos_i by rlap_spmm.h's chunk rule) / num_pos,  E_neg = (the same of neg_i) / num_neg,
//                   num_pos = N, num_neg = N G - N (G >= 2, formed in int64) or N (G == 1);  loss = E_neg - E_pos.
//   JSD backward    with the upstream gradient gup (a double):  d = 1 + e;  sigma(x) = (x >= 0 ? 1 / d : e / d) + nf, float32 IEEE
//                   operations;  w_ij = (float)(-(gup / num_pos) * sigma(-s_ij)) for the positive pair,
//                   (float)((gup / num_neg) * sigma(s_ij)) for a negative pair, 0 for a padding row or column.
//                   dh_i  = sum over j of w_ij g_j, float32 fmaf chains from +0 over the graph tiles in increasing order, inside a
//                   tile the graphs 32 t + reg_row(r, hf), r = 0 .. 15 outside, hf = 0, 1 inside; a graph >= G takes its turn as
//                   fmaf(0, 0, acc).  G == 1: dh_ik = fmaf(w_i, g_0k, +0), dneg_ik = fmaf(w'_i, g_0k, +0).
//                   dg_j  = float32 fmaf chains over the nodes from +0 per PART of the 32-node tiles (num_parts(N, G, F) contiguous
//                   parts, tiles [part_begin(p), part_begin(p + 1))); dg_j = 0 + part 0 + part 1 + ... in float32.
//                   G >= 2: inside tile t the nodes 32 t + reg_row(r, hf), r outside, hf inside; a node >= N takes its turn as
//                   fmaf(0, 0, acc).  G == 1: the nodes of the part in increasing order, node i adding fmaf(w_i, h_ik, acc) and
//                   then fmaf(w'_i, neg_ik, acc).
//   bootstrap       c_i = the chain of <ghat_{g(i)}, hhat_i>;  loss = (chunk rule over i of (double)c_i) / G.
//                   backward: Gh_ik = (gup / G) * (double)ghat_{g(i) k};  dot_i = sum over k in order of hhat_ik * Gh_ik;
//                   dh_ik = infonce::grad_in(Gh_ik, hhat_ik, dot_i, nrm_i, clamped).  No gradient for g.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rlap_infonce.h"
#include "rlap_spmm.h"
#include "rlap_tile32.h"

namespace rlap {
namespace g2l {

// a score tile (32 nodes x 32 graphs) is rlap_tile32.h's
using tile32::TILE;
using tile32::BLOCK_TILES;
using tile32::num_tiles;
using tile32::row_blocks;
using tile32::padded_rows;
using tile32::padded_features;
using tile32::reg_row;

constexpr int MAX_F = infonce::MAX_F;             // feature columns of a call
constexpr int64_t TARGET_GROUPS = 256;            // workgroups the dg pass aims at when G is small
constexpr int64_t VEC_PARTS = 1024;               // parts of the dg pass of a single graph, at most
constexpr int VEC_THREADS = 256;                  // rows of a block of the vector kernels, at most (one thread per row)
constexpr int64_t VEC_LDS_BYTES = 66 * 1024;      // LDS of a block of the vector kernels, at most

enum Call { JSD_FORWARD = 0, JSD_BACKWARD = 1, BOOT_FORWARD = 2, BOOT_BACKWARD = 3 };

// ---- parts
// the parts of the node tiles in the dg pass: a function of (N, G, F) alone (F does not enter today)
RLAP_SPMM_HD int64_t num_parts(int64_t N, int64_t G, int64_t F) {
    (void)F;
    const int64_t T = num_tiles(N);
    if (T < 1) return 1;
    if (G == 1) return T < VEC_PARTS ? T : VEC_PARTS;
    const int64_t rb = row_blocks(G);
    const int64_t p = (TARGET_GROUPS + rb - 1) / rb;
    return p < 1 ? 1 : (p > T ? T : p);
}
RLAP_SPMM_HD int64_t part_begin(int64_t N, int64_t G, int64_t F, int64_t p) { return p * num_tiles(N) / num_parts(N, G, F); }   // (T < 2^26, p <= 1024)

// the vector kernels (one graph, bootstrap): one thread per row, the rows of a block staged in LDS with an odd stride
RLAP_SPMM_HD int vec_stride(int64_t F) { return (int)(F | 1); }
RLAP_SPMM_HD int vec_rows(int64_t F) {
    int R = VEC_THREADS;
    while (R > TILE && (int64_t)R * vec_stride(F) * 4 > VEC_LDS_BYTES) R >>= 1;
    return R;
}
RLAP_SPMM_HD int64_t vec_blocks(int64_t N, int64_t F) { return (N + vec_rows(F) - 1) / vec_rows(F); }

// ---- the node -> graph map: the last graph j in [0, G) whose clamped offset is <= i.  Every value read from the table is clamped to
// [0, N] before it is compared, and the result lies in [0, G) whatever the table holds.
RLAP_SPMM_HD int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
RLAP_SPMM_HD int64_t graph_of(const int64_t* node_ptr, int64_t G, int64_t N, int64_t i) {
    int64_t lo = 0, hi = G;   // tab[lo] <= i < tab[hi] for a well-formed table
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (clampi(node_ptr[mid], 0, N) <= i) lo = mid; else hi = mid;
    }
    return lo;
}

RLAP_SPMM_HD int64_t num_pos(int64_t N) { return N; }
RLAP_SPMM_HD int64_t num_neg(int64_t N, int64_t G) { return G == 1 ? N : N * G - N; }   // (N, G < 2^31)

// ---- the arena: the pieces of each call, 256-byte aligned, in this order
enum Piece { P_MAP = 0, P_HFRAG, P_GFRAG, P_HROWS, P_GROWS, P_PARTIAL, P_W, P_GHAT, P_CSUM, P_COUNT };
struct Arena {
    int64_t off[P_COUNT];    // byte offset of a piece, -1 when the call has none
    int64_t size[P_COUNT];   // its bytes
    int64_t bytes;           // of the call
};
RLAP_SPMM_HD void take(Arena* A, int piece, int64_t bytes) {
    A->bytes = (A->bytes + 255) & ~(int64_t)255;
    A->off[piece] = A->bytes;
    A->size[piece] = bytes;
    A->bytes += bytes;
}
RLAP_SPMM_HD Arena arena(int call, int64_t N, int64_t G, int64_t F) {
    Arena A;
    for (int p = 0; p < P_COUNT; ++p) { A.off[p] = -1; A.size[p] = 0; }
    A.bytes = 0;
    const int64_t Np = padded_rows(N), Gp = padded_rows(G), Fp = padded_features(F), nc = spmm::num_chunks(N);
    const int64_t parts = num_parts(N, G, F);
    const bool back = call == JSD_BACKWARD || call == BOOT_BACKWARD;
    if (call == JSD_FORWARD || call == JSD_BACKWARD) {
        if (G >= 2) {
            take(&A, P_MAP, 4 * Np);
            take(&A, P_HFRAG, 4 * Np * Fp);
            take(&A, P_GFRAG, 4 * Gp * Fp);
            if (back) {
                take(&A, P_HROWS, 4 * Np * Fp);
                take(&A, P_GROWS, 4 * Gp * Fp);
                take(&A, P_PARTIAL, 4 * parts * Gp * Fp);
            }
        } else if (back) {
            take(&A, P_PARTIAL, 4 * parts * F);
            take(&A, P_W, 4 * 2 * N);
        }
        if (!back) take(&A, P_CSUM, 8 * 2 * nc);
    } else {
        take(&A, P_MAP, 4 * N);
        take(&A, P_GHAT, 4 * G * F);
        if (!back) take(&A, P_CSUM, 8 * nc);
    }
    A.bytes += 256;
    return A;
}

// ---- the values
RLAP_SPMM_HD float score_step(float acc, float x, float y) { return infonce::sim_step(acc, x, y); }

RLAP_SPMM_HD float clamp_abs(float s) {
    const float a = fabsf(s);
    return a < 64.0f ? a : 64.0f;   // (false for a NaN: 64)
}
RLAP_SPMM_HD float e_of(float s) { return infonce::expw(-clamp_abs(s)); }
RLAP_SPMM_HD float nonfinite(float s) { return s - s; }
RLAP_SPMM_HD double relu(double x) { return x < 0.0 ? 0.0 : x; }
// both terms of a score
RLAP_SPMM_HD void terms(float s, double* pos, double* neg) {
    const double v = log1p(((double)e_of(s) - 1.0) * 0.5);   // log((1 + e) / 2) = log1p(e) - ln 2, without the cancellation
    const double nf = (double)nonfinite(s);
    const double a = -(relu(-(double)s) + v);                // ln 2 - softplus(-s)
    const double b = relu((double)s) + v;                    // softplus(s) - ln 2
    *pos = a + nf;
    *neg = b + nf;
}
RLAP_SPMM_HD double pos_term(float s) { double p, n; terms(s, &p, &n); return p; }
RLAP_SPMM_HD double neg_term(float s) { double p, n; terms(s, &p, &n); return n; }

RLAP_SPMM_HD double jsd_loss(double total_pos, double total_neg, int64_t N, int64_t G) {
    const double ep = total_pos / (double)num_pos(N);
    const double en = total_neg / (double)num_neg(N, G);
    return en - ep;
}

RLAP_SPMM_HD float sigma(float x) {
    const float e = e_of(x);
    const float d = 1.0f + e;
    const float big = 1.0f / d;
    const float small = e / d;
    return (x >= 0.0f ? big : small) + nonfinite(x);
}
RLAP_SPMM_HD double pos_coef(double gup, int64_t N) { return -(gup / (double)num_pos(N)); }
RLAP_SPMM_HD double neg_coef(double gup, int64_t N, int64_t G) { return gup / (double)num_neg(N, G); }
// the weight of a pair: cp = pos_coef, cn = neg_coef
RLAP_SPMM_HD float weight(double cp, double cn, float s, bool positive) {
    const float arg = positive ? -s : s;
    const double c = positive ? cp : cn;
    return (float)(c * (double)sigma(arg));
}

RLAP_SPMM_HD double boot_loss(double total, int64_t G) { return total / (double)G; }
RLAP_SPMM_HD double boot_scale(double gup, int64_t G) { return gup / (double)G; }
RLAP_SPMM_HD double boot_grad_hat(double scale, float ghat) { return scale * (double)ghat; }

}  // namespace g2l
}  // namespace rlap
