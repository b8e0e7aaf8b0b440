// rlap_edgedrop.h -- centrality-adaptive edge dropping (rlap_edge_drop).  Two parts:
//   1. the rules as plain __host__ __device__ functions without any HIP dependency: tests/csrc/edgedrop_mirror.cc compiles them
//      with g++ and runs a whole call on the host; the kernels of rlap_edgedrop.hip read the same functions;
//   2. (HIP only) the interface between rlap_edgedrop.hip, which holds the kernels and their orchestration, and the C ABI in
//      rlap_api.hip, which owns the handle, its lock and its arena.
// The input is E rows (source, target) in any order; duplicates, loops and directed structure stay as they are.  All arithmetic is
// float64, every operation rounded on its own (the library and the mirror are built with contraction off), and every sum runs in
// an order that depends on the input alone:
//   list    the sum over a node's incoming rows, in input order of the rows, by rlap_edgeplan.h's rule: place k of the list goes to
//           lane k % 16, accumulator (k / 16) % 4, ascending k; per lane (a0 + a1) + (a2 + a3); an xor butterfly over 8, 4, 2, 1
//           lanes (list_sum);
//   tile    the nodes are cut into tiles of TILE = 256; the 256 values of a tile (0 past the last node) meet in an xor butterfly
//           over 32, 16, 8, 4, 2, 1 lanes inside each of the four waves, then (w0 + w1) + (w2 + w3) (tile_reduce);
//   total   the tile partials: lane i of 256 adds partials i, i + 256, ... in ascending order from the operation's identity, then
//           the 256 lanes meet as a tile does (total_reduce).  Maxima run through the same trees.
// Counts: in[v] / out[v] = the rows with target / source v; cnt = in for RLAP_DROP_SINK, out for RLAP_DROP_SOURCE.
// Centralities c[v]:
//   degree       the distinct u with a row (u, v) or (v, u), a loop counted once (an integer);
//   pagerank     x = 1; pr_iters times: z[u] = x[u] / out[u] (0 where out[u] = 0), x[v] = (1 - damp) * x[v] + damp * list_v(z);
//   eigenvector  x = 1 / sqrt(N); a step: y[v] = x[v] + list_v(x), nrm = sqrt(total(tile(y * y))), x' = y / nrm,
//                err = total(tile(|x' - x|)); stops after the step with err <= N * tol, or after max_iter steps;
//                c = max(x, 0) + 1e-8.  Duplicate rows count as often as they occur.
// Scores, with s[v] = log(c[v]) and a term taken only where cnt[v] > 0 (0 or the identity elsewhere):
//   smax = max s[v];  smean = total(cnt * s) / E;  w[v] = (smax - s[v]) / (smax - smean);  wmean = total(cnt * w) / E;
//   node_weight[v] = w[v] / wmean.
// Drop probability of row e in view k, t_e its target (sink) or source: uniform: q = p[k]; otherwise t = node_weight[t_e] * p[k],
// q = t < threshold ? t : threshold (so a NaN gives threshold).  Coin: u(k, e) below; the row is kept iff u >= q.
//
// Limits (RLAP_E_TOO_LARGE, never truncated): E < 2^31 - 1, num_nodes < 2^31, K <= 32.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "rlap_core.h"
#include "rlap_edgeplan.h"

namespace rlap {
namespace edgedrop {

constexpr int TILE = 256;             // nodes of a tile = threads of a workgroup
constexpr int WAVE = 64;
constexpr int ROW_TILE = 2048;        // rows a workgroup flips and compacts
constexpr int MAX_VIEWS = 32;
constexpr int64_t MAX_PR_ITERS = 100000, MAX_EVC_ITERS = 100000;
constexpr uint64_t COIN_SALT = 0x6564676564726F70ull;
enum { UNIFORM = 0, DEGREE = 1, PAGERANK = 2, EIGENVECTOR = 3, SCHEMES = 4 };

struct Add { RLAP_SPMM_HD double operator()(double a, double b) const { return a + b; } RLAP_SPMM_HD double identity() const { return 0.0; } };
struct Max { RLAP_SPMM_HD double operator()(double a, double b) const { return b > a ? b : a; } RLAP_SPMM_HD double identity() const { return -INFINITY; } };

RLAP_SPMM_HD int64_t tiles(int64_t n) { return (n + TILE - 1) / TILE; }
RLAP_SPMM_HD int64_t row_tiles(int64_t E) { return (E + ROW_TILE - 1) / ROW_TILE; }

// the four wave results of a tile
template <class Op> RLAP_SPMM_HD double combine_waves(Op op, double w0, double w1, double w2, double w3) { return op(op(w0, w1), op(w2, w3)); }

// ---- the coin
RLAP_SPMM_HD uint64_t coin_view(uint64_t seed, int k) { return mix64((seed + (uint64_t)k) ^ COIN_SALT); }
RLAP_SPMM_HD uint64_t coin_row(int64_t e) { return mix64((uint64_t)e); }
RLAP_SPMM_HD double coin_of(uint64_t view, uint64_t row) {
    const uint64_t z = mix64(view ^ row);
    return (double)(z >> 11) * 1.1102230246251565e-16;   // 2^-53
}
// u(k, e) = (mix64(mix64((seed + k) ^ COIN_SALT) ^ mix64(e)) >> 11) * 2^-53
RLAP_SPMM_HD double coin(uint64_t seed, int k, int64_t e) { return coin_of(coin_view(seed, k), coin_row(e)); }

// ---- the drop probability and the decision
RLAP_SPMM_HD double drop_prob(bool uniform, double node_weight, double p, double threshold) {
    if (uniform) return p;
    const double t = node_weight * p;
    return t < threshold ? t : threshold;
}
RLAP_SPMM_HD bool keeps(double u, double q) { return u >= q; }

// ---- per node
RLAP_SPMM_HD double pr_share(double x, int32_t out) { return out > 0 ? x / (double)out : 0.0; }
RLAP_SPMM_HD double pr_update(double x, double sum, double damp) {
    const double a = (1.0 - damp) * x, b = damp * sum;
    return a + b;
}
RLAP_SPMM_HD double evc_start(int64_t N) { return 1.0 / sqrt((double)N); }
RLAP_SPMM_HD double evc_finish(double x) { return (x > 0.0 ? x : 0.0) + 1e-8; }
RLAP_SPMM_HD bool evc_stops(double err, int64_t N, double tol) { return err <= (double)N * tol; }
RLAP_SPMM_HD double weighted_term(int32_t cnt, double v) { return cnt > 0 ? (double)cnt * v : 0.0; }
RLAP_SPMM_HD double max_term(int32_t cnt, double v) { return cnt > 0 ? v : -INFINITY; }
RLAP_SPMM_HD double score_w(double smax, double smean, double s) { return (smax - s) / (smax - smean); }

// bits of the degree sort's keys v * N + u
RLAP_SPMM_HD unsigned pair_key_bits(int64_t N) {
    unsigned b = 1;
    const uint64_t top = (uint64_t)N * (uint64_t)N;
    while (b < 64 && ((uint64_t)1 << b) < top) ++b;
    return b;
}

// ---- the host's form of the three sums (the kernels run the same functions lanes wide)
template <class Term>
inline double list_sum(int64_t n, Term term) {
    double acc[edgeplan::LANES][edgeplan::ACCS];
    for (int l = 0; l < edgeplan::LANES; ++l)
        for (int u = 0; u < edgeplan::ACCS; ++u) acc[l][u] = 0.0;
    for (int64_t k = 0; k < n; ++k) acc[edgeplan::lane_of(k)][edgeplan::acc_of(k)] += term(k);
    double v[edgeplan::LANES];
    for (int l = 0; l < edgeplan::LANES; ++l) v[l] = edgeplan::combine(acc[l]);
    for (int o = edgeplan::LANES / 2; o > 0; o >>= 1) {
        double t[edgeplan::LANES];
        for (int l = 0; l < edgeplan::LANES; ++l) t[l] = edgeplan::meet(v[l], v[l ^ o]);
        for (int l = 0; l < edgeplan::LANES; ++l) v[l] = t[l];
    }
    return v[0];
}

template <class Op>
inline double tile_reduce(Op op, const double (&in)[TILE]) {
    double v[TILE];
    for (int i = 0; i < TILE; ++i) v[i] = in[i];
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        double t[TILE];
        for (int i = 0; i < TILE; ++i) t[i] = op(v[i], v[i ^ o]);
        for (int i = 0; i < TILE; ++i) v[i] = t[i];
    }
    return combine_waves(op, v[0], v[WAVE], v[2 * WAVE], v[3 * WAVE]);
}

// tile t of value(i), i in [0, n)
template <class Op, class Value>
inline double tile_of(Op op, int64_t n, int64_t t, Value value) {
    double v[TILE];
    for (int i = 0; i < TILE; ++i) v[i] = t * TILE + i < n ? value(t * TILE + i) : op.identity();
    return tile_reduce(op, v);
}

template <class Op>
inline double total_reduce(Op op, const double* part, int64_t n) {
    double v[TILE];
    for (int i = 0; i < TILE; ++i) {
        double p = op.identity();
        for (int64_t t = i; t < n; t += TILE) p = op(p, part[t]);
        v[i] = p;
    }
    return tile_reduce(op, v);
}

}  // namespace edgedrop
}  // namespace rlap

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

namespace rlap {

struct EdgeDropArgs {
    const int64_t* src; const int64_t* dst; const double* w; int64_t E, N;
    int scheme, source;                        // source: cnt and the endpoint are the row's source
    double p[edgedrop::MAX_VIEWS]; int K;
    double threshold; uint64_t seed;
    double damp; int64_t pr_iters; double evc_tol; int64_t evc_max_iter;
    double* rows; int64_t cap; int64_t* ptr;   // (cap, 3) and [K + 1]
    uint8_t* mask; double* centrality; double* node_weight;   // optional: (K, E), [N], [N]
};
struct EdgeDropReport { int64_t rows_needed, launches; int32_t iters, converged, host_syncs; };

size_t edge_drop_bytes(int64_t E, int64_t N, int K, int scheme);
int edge_drop_run(hipStream_t stream, void* ws, size_t ws_bytes, const EdgeDropArgs& a, EdgeDropReport* rep);

}  // namespace rlap
#endif
