// markov_mirror.cc -- the Markov diffusion of one segment on the host, sparse, by the scalar rule of rlap_amd/csrc/rlap_markov.h (the
// header rlap_markov.hip includes) and in the device's order of operations: a node's rows are summed in row order, then the diagonal
// term; the pair {i, j} takes its value and its keep decision from the column of the smaller-ranked id; the row sums of the
// normalisation run in 64 strided partial sums and an xor butterfly, as k_pp_rowsum does.  Built with -ffp-contract=off it computes
// the device's bits (tests/markov_mirror.py loads it; tests/csrc/markov_main.cc is the stand-alone program for the sanitizers).
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <vector>

#include "rlap_markov.h"

namespace {

enum { MK_OK = 0, MK_BAD_ARG = 3, MK_NOT_SYMMETRIC = 5, MK_NOT_GROUPED = 12 };
constexpr int64_t TILE = 64;

struct Entry { int64_t ri, rj; double v; };
std::vector<double> g_raw, g_norm;   // the rows of the last call: [i, j, value]

}  // namespace

extern "C" {

int markov_max_order() { return rlap::markov::MAX_ORDER; }
int markov_final_copy(int order) { return rlap::markov::final_copy(order); }
int markov_valid(double alpha, int order, double eps) { return rlap::markov::valid(alpha, order, eps) ? 1 : 0; }

// One segment: sc (m, 3) rows [row id, column id, weight] grouped by column.  tiles / ntiles: the source tiles (64 consecutive
// columns in input order each) whose columns are computed; ntiles < 0: all of them.  Returns the number of kept rows (fetch them
// with markov_fetch) or a negative status.  With a subset of the tiles only the pairs whose smaller-ranked id lies in a computed
// column are returned, and the normalised values are not meaningful.
int64_t markov_run(const double* sc, int64_t m, int weighted, int self_loop, int zero_ok, double alpha, int order, double eps,
                   const int64_t* tiles, int64_t ntiles) {
    using namespace rlap;
    g_raw.clear(); g_norm.clear();
    if (!markov::valid(alpha, order, eps) || m < 0) return -MK_BAD_ARG;
    for (int64_t r = 0; r < m; ++r) {
        const double w = sc[3 * r + 2];
        if (weighted && !((zero_ok ? w >= 0.0 : w > 0.0) && w < INFINITY)) return -MK_BAD_ARG;
    }
    // blocks: runs of rows with one column id, in input order
    std::vector<int64_t> bstart, id;
    std::map<int64_t, int64_t> block_of;
    for (int64_t r = 0; r < m; ++r) {
        const int64_t c = (int64_t)sc[3 * r + 1];
        if (r == 0 || c != (int64_t)sc[3 * (r - 1) + 1]) {
            if (block_of.count(c)) return -MK_NOT_GROUPED;
            block_of[c] = (int64_t)id.size();
            id.push_back(c);
            bstart.push_back(r);
        }
    }
    bstart.push_back(m);
    const int64_t n = (int64_t)id.size();
    std::vector<int64_t> rb((size_t)m), blk((size_t)m), rank((size_t)n);
    for (int64_t b = 0; b < n; ++b)
        for (int64_t r = bstart[b]; r < bstart[b + 1]; ++r) {
            blk[r] = b;
            const auto it = block_of.find((int64_t)sc[3 * r]);
            if (it == block_of.end()) return -MK_NOT_SYMMETRIC;
            rb[r] = it->second;
        }
    { int64_t k = 0; for (const auto& kv : block_of) rank[kv.second] = k++; }   // (the map iterates in ascending id order)
    // degrees, coefficients
    std::vector<double> dinv((size_t)n), cdiag((size_t)n), a((size_t)m);
    for (int64_t b = 0; b < n; ++b) {
        double d = 0.0;
        for (int64_t r = bstart[b]; r < bstart[b + 1]; ++r) d += weighted ? sc[3 * r + 2] : 1.0;
        if (self_loop) d += 1.0;
        dinv[b] = markov::dinv(d);
        cdiag[b] = self_loop ? markov::diag(dinv[b]) : 0.0;
    }
    for (int64_t r = 0; r < m; ++r) a[r] = markov::coef(weighted ? sc[3 * r + 2] : 1.0, dinv[blk[r]], dinv[rb[r]]);
    // the columns
    std::vector<char> want((size_t)n, ntiles < 0 ? 1 : 0);
    for (int64_t t = 0; t < ntiles; ++t)
        for (int64_t j = tiles[t] * TILE; j < std::min(n, (tiles[t] + 1) * TILE); ++j) if (j >= 0) want[j] = 1;
    const double beta = markov::beta_of(alpha);
    std::vector<Entry> kept;
    std::vector<double> copy[2] = {std::vector<double>((size_t)n), std::vector<double>((size_t)n)};
    for (int64_t j = 0; j < n; ++j) {
        if (!want[j]) continue;
        for (int64_t i = 0; i < n; ++i) copy[0][i] = i == j ? 1.0 : 0.0;
        for (int mm = 0; mm <= order; ++mm) {
            const std::vector<double>& cur = copy[mm & 1];
            std::vector<double>& nxt = copy[(mm & 1) ^ 1];
            for (int64_t i = 0; i < n; ++i) {
                double acc = 0.0;
                for (int64_t r = bstart[i]; r < bstart[i + 1]; ++r) acc += a[r] * cur[rb[r]];
                acc += cdiag[i] * cur[i];
                nxt[i] = mm < order ? markov::step(acc, i == j, alpha, beta, order, mm) : markov::last(acc);
            }
        }
        const std::vector<double>& fin = copy[markov::final_copy(order)];
        for (int64_t i = 0; i < n; ++i) {
            if (rank[i] < rank[j] || !(fin[i] >= eps)) continue;
            kept.push_back({rank[i], rank[j], fin[i]});
            if (rank[i] != rank[j]) kept.push_back({rank[j], rank[i], fin[i]});
        }
    }
    std::sort(kept.begin(), kept.end(), [](const Entry& x, const Entry& y) { return x.ri != y.ri ? x.ri < y.ri : x.rj < y.rj; });
    // row sums as the device takes them: lane l sums entries l, l + 64, ... of the row, then an xor butterfly
    std::vector<double> dsinv((size_t)n, 0.0);
    std::vector<int64_t> id_of_rank((size_t)n);
    for (int64_t b = 0; b < n; ++b) id_of_rank[rank[b]] = id[b];
    for (size_t e0 = 0; e0 < kept.size();) {
        size_t e1 = e0;
        while (e1 < kept.size() && kept[e1].ri == kept[e0].ri) ++e1;
        double lane[64];
        for (int l = 0; l < 64; ++l) {
            double acc = 0.0;
            for (size_t e = e0 + (size_t)l; e < e1; e += 64) acc += kept[e].v;
            lane[l] = acc;
        }
        for (int o = 32; o > 0; o >>= 1) {
            double nw[64];
            for (int l = 0; l < 64; ++l) nw[l] = lane[l] + lane[l ^ o];
            for (int l = 0; l < 64; ++l) lane[l] = nw[l];
        }
        dsinv[kept[e0].ri] = lane[0] > 0.0 ? 1.0 / sqrt(lane[0]) : 0.0;
        e0 = e1;
    }
    for (const Entry& e : kept) {
        const double i = (double)id_of_rank[e.ri], j = (double)id_of_rank[e.rj];
        g_raw.push_back(i); g_raw.push_back(j); g_raw.push_back(e.v);
        g_norm.push_back(i); g_norm.push_back(j); g_norm.push_back(e.v * (dsinv[e.ri] * dsinv[e.rj]));
    }
    return (int64_t)kept.size();
}

// the rows of the last markov_run: raw (before normalisation) and normalised, (rows, 3) each
void markov_fetch(double* raw, double* norm) {
    std::copy(g_raw.begin(), g_raw.end(), raw);
    std::copy(g_norm.begin(), g_norm.end(), norm);
}

}  // extern "C"
