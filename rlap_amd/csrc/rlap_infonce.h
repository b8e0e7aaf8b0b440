// rlap_infonce.h -- the rule of the fused InfoNCE contrastive loss (rlap_infonce / rlap_infonce_backward, rlap_infonce.hip,
// DESIGN 4.15): every value of the call and the order of every sum.  Plain __host__ __device__ functions without any HIP dependency,
// as rlap_spmm.h: tests/csrc/infonce_mirror.cc compiles this file with g++ (contraction off, as the library) and computes the same
// bits; tests/csrc/infonce_main.cc runs the index arithmetic under the sanitizers; the kernels read the same functions.
//
// Inputs: a (anchor) and b (sample), (N, F) float32, and tau in [1/32, 1024].  The positive of row i is column i; every column, the
// positive included, is in the denominator (the L2L / G2G sampler with intraview_negs=False; with it on, the last section below).
//
//   normalisation   n2_i = sum over k = 0 .. F-1, in order, of (double)a_ik * (double)a_ik (product rounded, add rounded);
//                   nrm_i = max(sqrt(n2_i), 1e-12);  ah_ik = (float)((double)a_ik / nrm_i); the same for bh.  A zero row stays zero.
//   similarity      s_ij = the float32 fmaf chain over k = 0 .. F-1 in increasing k from +0: acc = fmaf(ah_ik, bh_jk, acc) -- what
//                   v_mfma_f32_32x32x2_f32 computes.  Zero columns behind F leave the chain's value as it is (fmaf(0, 0, x) = x; a
//                   -0 may become +0, and the sign of a zero s reaches no result: s enters as s - 1 and as c * s - inv_tau).
//   exponent        e_ij = expw((s_ij - 1) * (float)(1 / tau)): |s| <= 1 up to rounding, so the shift by 1 bounds the row maximum
//                   and no rescaling is needed; expw is written out below, its argument stays in [-64, 0] and e stays normal.
//   row sum         Z_i over the 32-column tiles of the samples, T = ceil(N / 32), dealt into num_parts(N) contiguous parts
//                   (tiles [part_begin(N, p), part_begin(N, p + 1))).  Inside a part two float64 sums run, one per lane half h:
//                   half h adds (double)e_ij of the columns j = 32 t + reg_row(r, h), r = 0 .. 15 in order, tile after tile
//                   (columns >= N are left out).  The part's sum is half 0 + half 1; Z_i = 0 + part 0 + part 1 + ... in order.
//                   The order depends on N alone.
//   row term        row_i = c * (double)s_ii - 1 / tau - log(Z_i), c = 1 / tau ("scaled", GCL's InfoNCE) or c = 1 ("raw",
//                   the reference's InfoNCEBatched, whose first term is not divided by tau).
//   loss            -(sum of row_i by rlap_spmm.h's chunk rule: chunks of 256 rows in order, chunk sums added in order) / N.
//   backward        with the upstream gradient g:  p_ij = e_ij * (float)(1 / Z_i);
//                   D_ik  = sum over j of p_ij bh_jk   (owner: the anchor i, stream: the samples j)
//                   D'_jk = sum over i of p_ij ah_ik   (owner: the sample j, stream: the anchors i)
//                   as float32 fmaf chains over the STREAM index, from +0 per part: the parts and their tiles as above; inside tile
//                   t the stream rows come in the order 32 t + reg_row(r, h), r = 0 .. 15 outside, h = 0, 1 inside (rows
//                   0 4 1 5 2 6 3 7 8 12 ...: a 32x32 accumulator tile fed to the next 32x32x2 MFMA as its A operand); a row
//                   >= N takes its turn as fmaf(0, 0, acc).  D = 0 + part 0 + part 1 + ... in float32.  Then in float64
//                   Gh_ik = gs * (c * bh_ik - (1 / tau) * D_ik), gs = -(g / N);  dot_i = sum over k in order of ah_ik * Gh_ik;
//                   ga_ik = (float)((Gh_ik - ah_ik * dot_i) / nrm_i), or (float)(Gh_ik / 1e-12) where sqrt(n2_i) < 1e-12 (the
//                   clamp of F.normalize passes no gradient to the norm).  The same for gb with the roles swapped.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rlap_spmm.h"
#include "rlap_tile32.h"

namespace rlap {
namespace infonce {

// a similarity tile is rlap_tile32.h's: its sizes, its register layout (reg_row) and the fragment image (frag_offset)
using tile32::TILE;
using tile32::BLOCK_TILES;
using tile32::num_tiles;
using tile32::row_blocks;
using tile32::padded_rows;
using tile32::padded_features;
using tile32::feature_tiles;
using tile32::reg_row;
using tile32::frag_offset;

constexpr int MAX_F = 512;                // feature columns of a call
constexpr int64_t TARGET_GROUPS = 256;    // workgroups a call aims at when N is small: what num_parts() is made from
constexpr double NORM_EPS = 1e-12;        // F.normalize's eps

RLAP_SPMM_HD bool tau_ok(double tau) { return tau >= 1.0 / 32.0 && tau <= 1024.0; }   // (false for a NaN)

// Which instance of a backward main kernel a call of nft = feature_tiles(F) takes (launch_backward_main of rlap_infonce.hip and of
// rlap_g2l.hip): k_in_main<NFT, .> and k_g2l_main<NFT, .> hold NFT accumulator tiles a wave and guard each with ft < nft, so the
// instance is the ladder's.  The launchers instantiate exactly its five; 0 for an nft outside [1, MAX_F / TILE].
static_assert(MAX_F / TILE == tile32::MAX_INSTANCE, "the ladder ends at MAX_F");
RLAP_SPMM_HD int main_instance(int nft) { return tile32::ladder_instance(nft); }

// The parts of the stream tiles: a function of N alone.  As many as bring the row blocks up to TARGET_GROUPS workgroups, at most
// one per tile.
RLAP_SPMM_HD int64_t num_parts(int64_t N) {
    const int64_t T = num_tiles(N), rb = row_blocks(N);
    if (T < 1) return 1;
    const int64_t p = (TARGET_GROUPS + rb - 1) / rb;
    return p < 1 ? 1 : (p > T ? T : p);
}
RLAP_SPMM_HD int64_t part_begin(int64_t N, int64_t p) { return p * num_tiles(N) / num_parts(N); }   // (T < 2^26, p <= 256)

// ---- the values
RLAP_SPMM_HD double norm2_step(double acc, float x) {
    const double t = (double)x * (double)x;
    return acc + t;
}
RLAP_SPMM_HD double norm2(const float* row, int64_t F) {
    double n2 = 0.0;
    for (int64_t k = 0; k < F; ++k) n2 = norm2_step(n2, row[k]);
    return n2;
}
RLAP_SPMM_HD double norm_of(double n2) {
    const double r = sqrt(n2);
    return r > NORM_EPS ? r : NORM_EPS;   // (a row that holds a NaN keeps it in hat(): the loss is then NaN, as in torch)
}
RLAP_SPMM_HD bool norm_clamped(double n2) { return sqrt(n2) < NORM_EPS; }
RLAP_SPMM_HD float hat(float x, double nrm) { return (float)((double)x / nrm); }

RLAP_SPMM_HD float sim_step(float acc, float x, float y) { return fmaf(x, y, acc); }

RLAP_SPMM_HD double inv_tau(double tau) { return 1.0 / tau; }
RLAP_SPMM_HD float inv_tau_f(double tau) { return (float)inv_tau(tau); }
RLAP_SPMM_HD float exp_arg(float s, float itf) { return (s - 1.0f) * itf; }

// exp(x) in float32 for x in [-64, 0] (any x in [-87, 88] in fact): n = x / ln 2 rounded to nearest by the 1.5 * 2^23 shift, r = x - n ln 2
// in two fmaf steps, the degree-7 Taylor polynomial in Horner form, 2^n added to the exponent bits.  IEEE operations only.
RLAP_SPMM_HD float expw(float x) {
    const float shift = 12582912.0f;
    const float t = x * 1.44269504088896341f + shift;
    const float n = t - shift;
    float r = fmaf(n, -0.693359375f, x);
    r = fmaf(n, 2.12194440e-4f, r);
    float p = 1.0f / 5040.0f;
    p = fmaf(p, r, 1.0f / 720.0f);
    p = fmaf(p, r, 1.0f / 120.0f);
    p = fmaf(p, r, 1.0f / 24.0f);
    p = fmaf(p, r, 1.0f / 6.0f);
    p = fmaf(p, r, 0.5f);
    p = fmaf(p, r, 1.0f);
    p = fmaf(p, r, 1.0f);
    int32_t bits;
    memcpy(&bits, &p, 4);
    bits += (int32_t)n * (1 << 23);
    memcpy(&p, &bits, 4);
    return p;
}

RLAP_SPMM_HD double row_term(double c, float sii, double itau, double Z) {
    const double t = c * (double)sii;
    const double u = t - itau;
    return u - log(Z);
}
RLAP_SPMM_HD double positive_coef(bool raw, double tau) { return raw ? 1.0 : inv_tau(tau); }
RLAP_SPMM_HD double loss_of(double total, int64_t N) { return -total / (double)N; }

RLAP_SPMM_HD float recip_z(double Z) { return (float)(1.0 / Z); }
RLAP_SPMM_HD float prob(float e, float rz) { return e * rz; }

RLAP_SPMM_HD double grad_scale(double g, int64_t N) { return -(g / (double)N); }
// the gradient with respect to a normalised element: `other` is the element of the other view's row, D the chain's sum
RLAP_SPMM_HD double grad_hat(double gs, double c, float other, double itau, float D) {
    const double t = c * (double)other;
    const double u = itau * (double)D;
    return gs * (t - u);
}
RLAP_SPMM_HD double dot_step(double acc, float h, double G) {
    const double t = (double)h * G;
    return acc + t;
}
RLAP_SPMM_HD float grad_in(double G, float h, double dot, double nrm, bool clamped) {
    if (clamped) return (float)(G / NORM_EPS);
    const double t = (double)h * dot;
    return (float)((G - t) / nrm);
}

// ---- the symmetric pair (rlap_infonce_pair / rlap_infonce_pair_backward): 0.5 * (l(a, b) + l(b, a)) from one pass
// over S.  fmaf(x, y, acc) == fmaf(y, x, acc), so the similarity of the second direction is bit for bit the transpose of the first's:
// s'_ji == s_ij and e'_ji == e_ij.  Normalisation, s_ij, expw, e_ij, row_term and the chunk rule are the ones above.
//
//   work split      a function of N alone.  The 128-row owner blocks (row_blocks(N)) are dealt into pair_groups(N) contiguous groups
//                   (blocks [pair_group_begin(N, g), pair_group_begin(N, g + 1))), the 32-column stream tiles into pair_parts(N)
//                   contiguous parts (tiles [pair_part_begin(N, p), pair_part_begin(N, p + 1))); one workgroup owns one (group, part).
//                   A part is walked in spans of at most PAIR_SPAN_TILES tiles (a part has one span below 262,145 rows).
//                   The partial sums are (pair_parts + pair_groups) x Np doubles: at most (512 + 16) Np.
//   row sum         Z_i: inside a span two float64 sums, one per lane half, exactly as above (tiles in order, registers in order,
//                   columns >= N left out); the span's sum is half 0 + half 1; the part's sum is 0 + span 0 + span 1 + ... (one
//                   span: half 0 + half 1, as above); Z_i = 0 + part 0 + part 1 + ... in order.
//   column sum      Zc_j = sum over the anchors i of e_ij, in float64:  Zc_j = 0 + group 0 + group 1 + ... in order; a group's sum
//                   starts from 0 and takes its row blocks in order; inside a row block the four 32-row owner tiles (the four waves)
//                   in order, each adding its tile's sum; a tile's sum is tree32 of (double)e_ij over its 32 owner rows, an owner
//                   row >= N entering as +0 (it is left out: a padded row has s = 0 and e = expw(-1/tau) != 0, so it is masked,
//                   and x + 0 = x for the non-negative x of these sums).  tree32: five rounds m = 1, 2, 4, 8, 16 of
//                   v[c] = v[c] + v[c ^ m] on all 32 values at once -- the butterfly x = x + shfl_xor(x, m); IEEE addition commutes,
//                   so after every round v[c] and v[c ^ m] hold the same bits, and the sum is v[0].  An owner tile behind the last
//                   adds +0.
//   row terms       rows_a_i = row_term(c, s_ii, 1/tau, Z_i);  rows_b_j = row_term(c, s_jj, 1/tau, Zc_j)
//   loss            0.5 * (loss_of(chunk-rule sum of rows_a, N) + loss_of(chunk-rule sum of rows_b, N))
//   backward        rza_i = recip_z(Z_i), rzb_j = recip_z(Zc_j);  w_ij = pair_weight(e_ij, rza_i, rzb_j) = e_ij * (rza_i + rzb_j) in
//                   float32 -- symmetric in the two reciprocals, so both owner kernels compute the same bits.  D and D' are the
//                   chains of the one-direction rule over num_parts(N) parts with w for p.  Gh = grad_hat(gs2, 2 c, other, 1/tau, D)
//                   with gs2 = pair_grad_scale(g, N) = -(g / (2 N)); dot, grad_in and the clamp as above.
constexpr int64_t PAIR_GROUPS = 16;           // groups of row blocks a call aims at
constexpr int64_t PAIR_WORKGROUPS = 512;      // (group, part) workgroups a call aims at
constexpr int64_t PAIR_SPAN_TILES = 256;      // stream tiles whose column sums a workgroup holds at once: 64 KB of doubles

RLAP_SPMM_HD int64_t pair_groups(int64_t N) {
    const int64_t rb = row_blocks(N);
    return rb < 1 ? 1 : (rb < PAIR_GROUPS ? rb : PAIR_GROUPS);
}
RLAP_SPMM_HD int64_t pair_group_begin(int64_t N, int64_t g) { return g * row_blocks(N) / pair_groups(N); }   // (RB < 2^24, g <= 16)
RLAP_SPMM_HD int64_t pair_parts(int64_t N) {
    const int64_t T = num_tiles(N), g = pair_groups(N);
    if (T < 1) return 1;
    const int64_t p = (PAIR_WORKGROUPS + g - 1) / g;
    return p > T ? T : p;
}
RLAP_SPMM_HD int64_t pair_part_begin(int64_t N, int64_t p) { return p * num_tiles(N) / pair_parts(N); }      // (T < 2^26, p <= 512)
// the most stream tiles of a span of any part: what the forward kernel's column array is sized by
RLAP_SPMM_HD int64_t pair_span_tiles(int64_t N) {
    const int64_t T = num_tiles(N), P = pair_parts(N);
    const int64_t longest = (T + P - 1) / P;   // (no part is longer: p T / P is floored at both ends)
    return longest < PAIR_SPAN_TILES ? (longest < 1 ? 1 : longest) : PAIR_SPAN_TILES;
}

// tree32 on 32 values held in an array (what the butterfly does on 32 lanes)
RLAP_SPMM_HD double tree32(const double* x) {
    double v[TILE], w[TILE];
    for (int c = 0; c < TILE; ++c) v[c] = x[c];
    for (int m = 1; m < TILE; m <<= 1) {
        for (int c = 0; c < TILE; ++c) w[c] = v[c] + v[c ^ m];
        for (int c = 0; c < TILE; ++c) v[c] = w[c];
    }
    return v[0];
}

RLAP_SPMM_HD double pair_loss_of(double total_a, double total_b, int64_t N) { return 0.5 * (loss_of(total_a, N) + loss_of(total_b, N)); }
RLAP_SPMM_HD float pair_weight(float e, float rz_own, float rz_str) { return e * (rz_own + rz_str); }
RLAP_SPMM_HD double pair_grad_scale(double g, int64_t N) { return -(g / (2.0 * (double)N)); }
RLAP_SPMM_HD double pair_positive_coef(bool raw, double tau) { return 2.0 * positive_coef(raw, tau); }   // 2 c: exact

// ---- intraview negatives (rlap_infonce_intra / rlap_infonce_pair_intra and their backward calls): the sampler with
// intraview_negs=True.  Row i of a view is contrasted with the rows of the other view AND with rows of its own view, the set I(i):
// every j != i (INTRA_MASKED: GCL's InfoNCE under the sampler's masks) or every j (INTRA_ALL: the reference's InfoNCEBatched, which
// never reads the masks and so counts the row's similarity with itself).  Normalisation, the chain s, exp_arg, expw, row_term, the
// chunk rule, grad_hat, dot, grad_in and the clamp are the ones above; the positive stays s^ab_ii.
//
//   intraview s, e  s^aa_ij = the chain over k of fmaf(ah_jk, ah_ik, acc) (the stream row first, as above; the order of the two does
//                   not reach the bits), e^aa_ij = expw(exp_arg(s^aa_ij, itf)), so e^aa_ij == e^aa_ji bit for bit.  s^aa_ii is a
//                   float32 chain of squares near 1 and may exceed it by a few roundings: exp_arg is then a few ulps above 0 times
//                   1 / tau <= 32, far inside the range expw is valid on ([-87, 88]), and e^aa_ii is 1 up to those roundings.
//   intraview sum   intra_a_i over the SAME parts and tiles as the row sum above (num_parts(N), part_begin) with both rows taken from
//                   ah: inside a part two float64 sums, one per lane half, registers in order, tile after tile; columns >= N are
//                   left out, and so is column i under INTRA_MASKED; the part's sum is half 0 + half 1.
//   one-way Z       Z_i = 0 + ab part 0 + ab part 1 + ... + aa part 0 + aa part 1 + ...: the parts of the row sum above in order,
//                   then the parts of the intraview sum in order, one float64 chain.
//   pair Z, Zc      Z_i  = 0 + the pair's parts of the row sum in order (pair_parts(N)) + the parts of intra_a in order;
//                   Zc_j = 0 + the pair's groups of the column sum in order (pair_groups(N)) + the parts of intra_b in order.
//   backward        one-way, the anchor owns:  D_ik = sum_j prob(e^ab_ij, rz_i) bh_jk + sum over j in I(i) of
//                   pair_weight(e^aa_ij, rz_i, rz_j) ah_jk -- row j's intraview sum reaches ah_i with the same e, so both fold into one
//                   weight; j = i under INTRA_ALL is pair_weight(e_ii, rz_i, rz_i), which the same expression yields.  ONE float32
//                   accumulator a part: inside part p the chain runs from +0 over the part's tiles of bh (the order above), then
//                   over the SAME tiles of ah in the same order; D = 0 + part 0 + part 1 + ... as above.  A stream row >= N takes
//                   its turn as fmaf(0, 0, acc); the masked row j = i takes its turn as fmaf(0, ah_ik, acc), which leaves acc as it
//                   is.  gb is the sample-owner chain above with rz from the new Z.
//                   pair: D^a_ik = sum_j pair_weight(e^ab_ij, rza_i, rzb_j) bh_jk + sum over j in I(i) of
//                   pair_weight(e^aa_ij, rza_i, rza_j) ah_jk in the same one-accumulator order; D^b with the roles swapped (e^bb, rzb).
// Every order is a function of N alone.
enum { INTRA_NONE = 0, INTRA_MASKED = 1, INTRA_ALL = 2 };
RLAP_SPMM_HD bool intra_ok(int intraview) { return intraview == INTRA_MASKED || intraview == INTRA_ALL; }
// whether column j is in I(i)
RLAP_SPMM_HD bool intra_member(int intraview, int64_t i, int64_t j) { return intraview == INTRA_ALL || i != j; }
// the parts a forward call keeps: the row sum's, then the intraview sum's (one-way); the pair adds 2 num_parts to its own
RLAP_SPMM_HD int64_t intra_z_parts(int64_t N) { return 2 * num_parts(N); }

}  // namespace infonce
}  // namespace rlap
