// nodesample_mirror.cc -- host mirror of rlap_node_sample: a whole call on the host through the functions of
// rlap_amd/csrc/rlap_nodesample.h, the same ones rlap_nodesample.hip's kernels read.  Built by tests/nodesample_mirror.py with g++
// (contraction off, as the library); tests/csrc/nodesample_main.cc runs it as a stand-alone program under the sanitizers.
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "rlap_nodesample.h"

using namespace rlap;
using namespace rlap::nodesample;

namespace {

enum { REFUSE_RANGE = 2, REFUSE_BAD_ARG = 3, REFUSE_TOO_LARGE = 9 };

}  // namespace

extern "C" {

double nodesample_u_node(uint64_t seed, int k, int64_t v) { return u_node(node_view(seed, k), v); }
double nodesample_u_walk(uint64_t seed, int k, int64_t i, int64_t t, int64_t walk_length) { return u_walk(walk_view(seed, k), i, t, walk_length); }
int64_t nodesample_pick(double u, int64_t n) { return pick(u, n); }
int nodesample_row_tile() { return ROW_TILE; }
int nodesample_max_views() { return MAX_VIEWS; }
int64_t nodesample_max_walk_length() { return MAX_WALK_LENGTH; }

// The whole call.  rows: (K * E, 3); ptr: [K + 1]; node_mask: (K, N) or null; walks: (sum of seeds, walk_length + 1) or null.
// Returns the kept rows of all views, or minus the status of a refusal.
int64_t nodesample_run(const int64_t* src, const int64_t* dst, const double* w, int64_t E, int64_t N, int scheme, const double* p,
                       const int64_t* num_seeds, int64_t K, int64_t walk_length, uint64_t seed, double* rows, int64_t* ptr,
                       uint8_t* node_mask, int64_t* walks) {
    if (E < 0 || N < 0 || (E > 0 && (!src || !dst)) || K < 1 || !ptr || (E > 0 && !rows)) return -REFUSE_BAD_ARG;
    if (scheme < 0 || scheme >= SCHEMES) return -REFUSE_BAD_ARG;
    const bool walk = scheme == WALK;
    if (walk ? !num_seeds : !p) return -REFUSE_BAD_ARG;
    if (!walk && walks) return -REFUSE_BAD_ARG;
    if (E >= INT32_MAX || N >= (int64_t)1 << 31 || K > MAX_VIEWS) return -REFUSE_TOO_LARGE;
    int64_t walkers = 0;
    for (int64_t k = 0; k < K; ++k) {
        if (walk) {
            if (num_seeds[k] < 0) return -REFUSE_BAD_ARG;
            if (num_seeds[k] >= (int64_t)1 << 31) return -REFUSE_TOO_LARGE;
            walkers += num_seeds[k];
        } else if (!(p[k] >= 0.0 && p[k] <= 1.0)) {
            return -REFUSE_BAD_ARG;
        }
    }
    if (walk && (walk_length < 0 || walk_length > MAX_WALK_LENGTH || (walkers > 0 && N == 0))) return -REFUSE_BAD_ARG;
    for (int64_t e = 0; e < E; ++e)
        if (src[e] < 0 || src[e] >= N || dst[e] < 0 || dst[e] >= N) return -REFUSE_RANGE;
    // the lists of outgoing rows, in input order
    std::vector<int64_t> lo, hi;
    std::vector<int32_t> tgts;
    if (walk) {
        std::vector<int64_t> cnt(N + 1, 0);
        for (int64_t e = 0; e < E; ++e) ++cnt[src[e] + 1];
        for (int64_t v = 0; v < N; ++v) cnt[v + 1] += cnt[v];
        lo.assign(cnt.begin(), cnt.begin() + N);
        hi = lo;
        tgts.assign(E, 0);
        for (int64_t e = 0; e < E; ++e) tgts[hi[src[e]]++] = (int32_t)dst[e];   // (stable: input order inside a list)
    }
    const int64_t W = set_words(N);
    std::vector<uint64_t> bits(W > 0 ? W : 1);
    int64_t total = 0, first = 0;
    for (int64_t k = 0; k < K; ++k) {
        ptr[k] = total;
        std::fill(bits.begin(), bits.end(), 0);
        if (walk) {
            const uint64_t view = walk_view(seed, (int)k);
            for (int64_t i = 0; i < num_seeds[k]; ++i) {
                int64_t* out = walks ? walks + (first + i) * (walk_length + 1) : nullptr;
                int64_t v = walk_start(view, i, walk_length, N);
                bits[v >> 6] |= (uint64_t)1 << (v & 63);
                if (out) out[0] = v;
                for (int64_t t = 1; t <= walk_length; ++t) {
                    const int64_t d = hi[v] - lo[v];
                    if (d > 0) v = tgts[lo[v] + walk_place(view, i, t, walk_length, d)];
                    bits[v >> 6] |= (uint64_t)1 << (v & 63);
                    if (out) out[t] = v;
                }
            }
            first += num_seeds[k];
        } else {
            const uint64_t view = node_view(seed, (int)k);
            for (int64_t v = 0; v < N; ++v)
                if (node_kept(view, node_hash(v), p[k])) bits[v >> 6] |= (uint64_t)1 << (v & 63);
        }
        if (node_mask)
            for (int64_t v = 0; v < N; ++v) node_mask[k * N + v] = set_test(bits.data(), v) ? 1 : 0;
        for (int64_t e = 0; e < E; ++e) {
            if (!set_test(bits.data(), src[e]) || !set_test(bits.data(), dst[e])) continue;
            rows[3 * total] = (double)src[e]; rows[3 * total + 1] = (double)dst[e]; rows[3 * total + 2] = w ? w[e] : 1.0;
            ++total;
        }
    }
    ptr[K] = total;
    return total;
}

}  // extern "C"
