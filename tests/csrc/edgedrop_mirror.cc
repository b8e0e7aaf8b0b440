// edgedrop_mirror.cc -- host mirror of rlap_edge_drop: a whole call on the host through the functions of
// rlap_amd/csrc/rlap_edgedrop.h, the same ones rlap_edgedrop.hip's kernels read.  Built by tests/edgedrop_mirror.py with g++
// (contraction off, as the library); tests/csrc/edgedrop_main.cc runs it as a stand-alone program under the sanitizers.
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "rlap_edgedrop.h"

using namespace rlap;
using namespace rlap::edgedrop;

namespace {

enum { REFUSE_RANGE = 2, REFUSE_BAD_ARG = 3, REFUSE_TOO_LARGE = 9 };

struct Lists {
    std::vector<int64_t> lo, hi;    // [N]: the list of v is srcs[lo[v] .. hi[v])
    std::vector<int32_t> srcs;      // [E] the sources, by target, in input order
};

Lists lists_by_target(const int64_t* src, const int64_t* dst, int64_t E, int64_t N) {
    Lists L;
    L.lo.assign(N, 0); L.hi.assign(N, 0); L.srcs.assign(E, 0);
    std::vector<int64_t> cnt(N + 1, 0);
    for (int64_t e = 0; e < E; ++e) ++cnt[dst[e] + 1];
    for (int64_t v = 0; v < N; ++v) cnt[v + 1] += cnt[v];
    for (int64_t v = 0; v < N; ++v) { L.lo[v] = cnt[v]; L.hi[v] = cnt[v]; }
    for (int64_t e = 0; e < E; ++e) L.srcs[L.hi[dst[e]]++] = (int32_t)src[e];   // (stable: input order inside a list)
    return L;
}

double list_of(const Lists& L, int64_t v, const std::vector<double>& x) {
    const int64_t s = L.lo[v];
    return list_sum(L.hi[v] - s, [&](int64_t k) { return x[L.srcs[s + k]]; });
}

template <class Op, class Value>
double total_of(Op op, int64_t N, Value value) {
    std::vector<double> part(tiles(N));
    for (int64_t t = 0; t < tiles(N); ++t) part[t] = tile_of(op, N, t, value);
    return total_reduce(op, part.data(), (int64_t)part.size());
}

}  // namespace

extern "C" {

double edgedrop_coin(uint64_t seed, int k, int64_t e) { return coin(seed, k, e); }
int edgedrop_tile() { return TILE; }
int edgedrop_row_tile() { return ROW_TILE; }
int edgedrop_max_views() { return MAX_VIEWS; }
unsigned edgedrop_pair_key_bits(int64_t N) { return pair_key_bits(N); }

// The whole call.  rows: (K * E, 3); ptr: [K + 1]; mask, q, u: (K, E) or null; centrality, node_weight: [N] or null.  Returns the
// kept rows of all views, or minus the status of a refusal.
int64_t edgedrop_run(const int64_t* src, const int64_t* dst, const double* w, int64_t E, int64_t N, int scheme, int source, const double* p,
                     int64_t K, double threshold, uint64_t seed, double damp, int64_t pr_iters, double evc_tol, int64_t evc_max_iter,
                     double* rows, int64_t* ptr, uint8_t* mask, double* q_out, double* u_out, double* centrality, double* node_weight,
                     int32_t* iters, int32_t* converged) {
    if (E < 0 || N < 0 || (E > 0 && (!src || !dst)) || !p || K < 1 || !ptr || (E > 0 && !rows)) return -REFUSE_BAD_ARG;
    if (scheme < 0 || scheme >= SCHEMES || (source & ~1)) return -REFUSE_BAD_ARG;
    if (E >= INT32_MAX || N >= (int64_t)1 << 31 || K > MAX_VIEWS) return -REFUSE_TOO_LARGE;
    if (!(threshold >= 0.0 && threshold <= 1.0)) return -REFUSE_BAD_ARG;
    for (int64_t k = 0; k < K; ++k)
        if (!(p[k] >= 0.0 && p[k] <= 1.0)) return -REFUSE_BAD_ARG;
    if (scheme == PAGERANK && (!(damp >= 0.0 && damp <= 1.0) || pr_iters < 0)) return -REFUSE_BAD_ARG;
    if (scheme == EIGENVECTOR && (!(evc_tol >= 0.0) || !std::isfinite(evc_tol) || evc_max_iter < 1)) return -REFUSE_BAD_ARG;
    if ((scheme == PAGERANK && pr_iters > MAX_PR_ITERS) || (scheme == EIGENVECTOR && evc_max_iter > MAX_EVC_ITERS)) return -REFUSE_TOO_LARGE;
    for (int64_t e = 0; e < E; ++e)
        if (src[e] < 0 || src[e] >= N || dst[e] < 0 || dst[e] >= N) return -REFUSE_RANGE;
    if (iters) *iters = scheme == PAGERANK ? (int32_t)pr_iters : 0;
    if (converged) *converged = 1;
    const bool scored = scheme != UNIFORM && E > 0 && N > 0;
    std::vector<double> c(N, 0.0), nw(N, 0.0);
    if (scored) {
        std::vector<int32_t> in(N, 0), out(N, 0);
        for (int64_t e = 0; e < E; ++e) { ++in[dst[e]]; ++out[src[e]]; }
        const std::vector<int32_t>& cnt = source ? out : in;
        if (scheme == DEGREE) {
            std::vector<uint64_t> keys(2 * E);
            for (int64_t e = 0; e < E; ++e) {
                keys[2 * e] = (uint64_t)dst[e] * (uint64_t)N + (uint64_t)src[e];
                keys[2 * e + 1] = (uint64_t)src[e] * (uint64_t)N + (uint64_t)dst[e];
            }
            std::sort(keys.begin(), keys.end());
            for (int64_t i = 0; i < 2 * E; ++i)
                if (i == 0 || keys[i] != keys[i - 1]) c[keys[i] / (uint64_t)N] += 1.0;
        } else {
            const Lists L = lists_by_target(src, dst, E, N);
            if (scheme == PAGERANK) {
                std::vector<double> z(N);
                std::fill(c.begin(), c.end(), 1.0);
                for (int64_t it = 0; it < pr_iters; ++it) {
                    for (int64_t v = 0; v < N; ++v) z[v] = pr_share(c[v], out[v]);
                    for (int64_t v = 0; v < N; ++v) c[v] = pr_update(c[v], list_of(L, v, z), damp);
                }
            } else {
                std::vector<double> x(N, evc_start(N)), y(N);
                int32_t done = 0, steps = 0;
                for (int64_t it = 0; it < evc_max_iter && !done; ++it) {
                    for (int64_t v = 0; v < N; ++v) y[v] = x[v] + list_of(L, v, x);
                    const double nrm = sqrt(total_of(Add(), N, [&](int64_t v) { return y[v] * y[v]; }));
                    std::vector<double> d(N);
                    for (int64_t v = 0; v < N; ++v) {
                        const double xn = y[v] / nrm;
                        d[v] = fabs(xn - x[v]);
                        x[v] = xn;
                    }
                    const double err = total_of(Add(), N, [&](int64_t v) { return d[v]; });
                    ++steps;
                    if (evc_stops(err, N, evc_tol)) done = 1;
                }
                for (int64_t v = 0; v < N; ++v) c[v] = evc_finish(x[v]);
                if (iters) *iters = steps;
                if (converged) *converged = done;
            }
        }
        std::vector<double> s(N), wv(N);
        for (int64_t v = 0; v < N; ++v) s[v] = log(c[v]);
        const double smax = total_of(Max(), N, [&](int64_t v) { return max_term(cnt[v], s[v]); });
        const double smean = total_of(Add(), N, [&](int64_t v) { return weighted_term(cnt[v], s[v]); }) / (double)E;
        for (int64_t v = 0; v < N; ++v) wv[v] = score_w(smax, smean, s[v]);
        const double wmean = total_of(Add(), N, [&](int64_t v) { return weighted_term(cnt[v], wv[v]); }) / (double)E;
        for (int64_t v = 0; v < N; ++v) nw[v] = wv[v] / wmean;
    }
    if (centrality) std::copy(c.begin(), c.end(), centrality);
    if (node_weight) std::copy(nw.begin(), nw.end(), node_weight);
    int64_t total = 0;
    for (int64_t k = 0; k < K; ++k) {
        ptr[k] = total;
        const uint64_t view = coin_view(seed, (int)k);
        for (int64_t e = 0; e < E; ++e) {
            const double q = drop_prob(scheme == UNIFORM, scored ? nw[source ? src[e] : dst[e]] : 0.0, p[k], threshold);
            const double u = coin_of(view, coin_row(e));
            const bool keep = keeps(u, q);
            if (q_out) q_out[k * E + e] = q;
            if (u_out) u_out[k * E + e] = u;
            if (mask) mask[k * E + e] = keep ? 1 : 0;
            if (!keep) continue;
            rows[3 * total] = (double)src[e]; rows[3 * total + 1] = (double)dst[e]; rows[3 * total + 2] = w ? w[e] : 1.0;
            ++total;
        }
    }
    ptr[K] = total;
    return total;
}

}  // extern "C"
