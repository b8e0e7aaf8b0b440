// edgeadd_mirror.cc -- host mirror of rlap_edge_add: a whole call on the host through the functions of
// rlap_amd/csrc/rlap_edgeadd.h, the same ones rlap_edgeadd.hip's kernels read.  Built by tests/edgeadd_mirror.py with g++
// (contraction off, as the library); tests/csrc/edgeadd_main.cc runs it as a stand-alone program under the sanitizers.
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "rlap_edgeadd.h"

using namespace rlap;
using namespace rlap::edgeadd;

namespace {

enum { REFUSE_RANGE = 2, REFUSE_BAD_ARG = 3, REFUSE_TOO_LARGE = 9 };

}  // namespace

extern "C" {

double edgeadd_u_add(uint64_t seed, int k, int64_t i, int c) { return u_add(add_view(seed, k), i, c); }
int64_t edgeadd_draw(uint64_t seed, int k, int64_t i, int c, int64_t N) { return draw(add_view(seed, k), i, c, N); }
unsigned edgeadd_id_bits(int64_t N) { return id_bits(N); }
uint64_t edgeadd_pair_key(int64_t s, int64_t t, int64_t N) { return pair_key(s, t, id_bits(N)); }
int edgeadd_one_sort(int64_t N, int K) { return one_sort(N, K) ? 1 : 0; }
int edgeadd_row_tile() { return ROW_TILE; }
int edgeadd_max_views() { return MAX_VIEWS; }

// The whole call.  rows: (K * E + sum of num_add, 3); ptr: [K + 1]; added: (sum of num_add, 2) or null; aptr: [K + 1] or null;
// stats: null or [input_distinct, input_sorted].  Returns the rows of all views, or minus the status of a refusal.
int64_t edgeadd_run(const int64_t* src, const int64_t* dst, const double* w, int64_t E, int64_t N, const int64_t* num_add, int64_t K,
                    uint64_t seed, int coalesce, double* rows, int64_t* ptr, int64_t* added, int64_t* aptr, int64_t* stats) {
    if (E < 0 || N < 0 || (E > 0 && (!src || !dst)) || !num_add || K < 1 || !ptr || !added != !aptr) return -REFUSE_BAD_ARG;
    if (E >= INT32_MAX || N >= (int64_t)1 << 31 || K > MAX_VIEWS) return -REFUSE_TOO_LARGE;
    int64_t all_added = 0;
    for (int64_t k = 0; k < K; ++k) {
        if (num_add[k] < 0) return -REFUSE_BAD_ARG;
        if (num_add[k] >= INT32_MAX - E) return -REFUSE_TOO_LARGE;
        all_added += num_add[k];
    }
    if (all_added > 0 && N < 2) return -REFUSE_BAD_ARG;
    if ((E > 0 || all_added > 0) && !rows) return -REFUSE_BAD_ARG;
    for (int64_t e = 0; e < E; ++e)
        if (src[e] < 0 || src[e] >= N || dst[e] < 0 || dst[e] >= N) return -REFUSE_RANGE;
    const unsigned b = id_bits(N);
    // list A: the distinct keys of the input, each with the sum of its rows in input order
    std::vector<uint64_t> akey;
    std::vector<double> asum;
    bool sorted = true;
    if (coalesce) {
        std::vector<uint64_t> key(E);
        for (int64_t e = 0; e < E; ++e) key[e] = pair_key(src[e], dst[e], b);
        for (int64_t e = 1; e < E; ++e) sorted = sorted && key[e - 1] <= key[e];
        std::vector<int64_t> order(E);
        std::iota(order.begin(), order.end(), (int64_t)0);
        std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key[x] < key[y]; });
        for (int64_t p = 0; p < E; ++p) {
            const int64_t e = order[p];
            if (p == 0 || key[e] != akey.back()) { akey.push_back(key[e]); asum.push_back(0.0); }
            asum.back() = run_add(asum.back(), w ? w[e] : 1.0);
        }
    }
    if (stats) { stats[0] = (int64_t)akey.size(); stats[1] = coalesce && sorted ? 1 : 0; }
    int64_t total = 0, first = 0;
    for (int64_t k = 0; k < K; ++k) {
        ptr[k] = total;
        if (aptr) aptr[k] = first;
        const uint64_t view = add_view(seed, (int)k);
        std::vector<uint64_t> bkey(num_add[k]);
        for (int64_t i = 0; i < num_add[k]; ++i) {
            const int64_t s = draw(view, i, 0, N), t = draw(view, i, 1, N);
            if (added) { added[2 * (first + i)] = s; added[2 * (first + i) + 1] = t; }
            bkey[i] = pair_key(s, t, b);
        }
        first += num_add[k];
        if (!coalesce) {
            for (int64_t e = 0; e < E; ++e, ++total) {
                rows[3 * total] = (double)src[e]; rows[3 * total + 1] = (double)dst[e]; rows[3 * total + 2] = w ? w[e] : 1.0;
            }
            for (int64_t i = 0; i < num_add[k]; ++i, ++total) {
                rows[3 * total] = (double)key_source(bkey[i], b); rows[3 * total + 1] = (double)key_target(bkey[i], b); rows[3 * total + 2] = 1.0;
            }
            continue;
        }
        // list B: the view's distinct added keys and their counts; then the merge, A first on ties
        std::sort(bkey.begin(), bkey.end());
        std::vector<uint64_t> bk;
        std::vector<int64_t> bc;
        for (uint64_t key : bkey) {
            if (bk.empty() || bk.back() != key) { bk.push_back(key); bc.push_back(0); }
            ++bc.back();
        }
        size_t ai = 0, bi = 0;
        while (ai < akey.size() || bi < bk.size()) {
            const bool from_a = ai < akey.size() && (bi >= bk.size() || takes_a(akey[ai], bk[bi]));
            const uint64_t key = from_a ? akey[ai] : bk[bi];
            double s_in = 0.0;
            int64_t c_add = 0;
            if (from_a) s_in = asum[ai++];
            if (bi < bk.size() && bk[bi] == key) c_add = bc[bi++];
            rows[3 * total] = (double)key_source(key, b); rows[3 * total + 1] = (double)key_target(key, b); rows[3 * total + 2] = weight(s_in, c_add);
            ++total;
        }
    }
    ptr[K] = total;
    if (aptr) aptr[K] = first;
    return total;
}

}  // extern "C"
