// Host mirror of the fused bias, activation and dropout pass (tests/test_rowops_cpu.py, tests/test_gpu_rowops.py): every value and
// every coin come from rlap_amd/csrc/rlap_rowops.h, compiled with g++ and contraction off, so that it computes the bits the kernels
// compute.  The loops below restate only the ORDER the header fixes: the chunk rule over the rows of a column, the layers in order,
// the columns in order.  tests/csrc/rowops_main.cc includes this file.
#include <cstdint>
#include <vector>

#include "rlap_rowops.h"

using namespace rlap;

namespace {

const auto one = [](int64_t) { return 1.0; };

template <class Coef, class Feat>
double rule_sum(int64_t n, Coef c, Feat x) { return spmm::list_sum(n, c, x, false, 0.0, 0.0); }

rowops::Col col_of(int64_t k, const float* b, const float* slope, int flags) {
    rowops::Col c{};
    c.b = b ? (double)b[k] : 0.0;
    c.a = (flags & rowops::ACT_PRELU) ? (double)slope[(flags & rowops::SLOPE_PER_CHANNEL) ? k : 0] : 0.0;
    return c;
}

}  // namespace

extern "C" {

int64_t rowops_const(int which) {
    switch (which) {
        case 0: return norm::MAX_GRID;
        case 1: return norm::GROUP_WAVES;
        case 2: return rowops::MAX_F;
        case 3: return spmm::CHUNK;
        case 4: return (int64_t)(rowops::COIN_SALT >> 32);
        case 5: return (int64_t)(rowops::COIN_SALT & 0xFFFFFFFFull);
        default: return -1;
    }
}
int rowops_args_ok(int64_t L, int64_t N, int64_t F, int flags, int has_slope, double p) {
    return rowops::args_ok(L, N, F, flags, has_slope != 0, p) ? 1 : 0;
}
uint32_t rowops_threshold(double p, int flags) { return rowops::threshold(p, flags); }
double rowops_scale(uint32_t T) { return rowops::scale(T); }
int rowops_split_of(int64_t items, int sums) { return rowops::split_of(items, sums != 0); }
int64_t rowops_backward_bytes(int64_t L, int64_t N, int64_t F, int want_bias, int want_slope) {
    return rowops::backward_bytes(L, N, F, rowops::planes_of(want_bias != 0, want_slope != 0));
}
// keep (L, N, F) bytes: 1 where the element is kept
void rowops_mask(int64_t L, int64_t N, int64_t F, double p, uint64_t seed, int flags, uint8_t* keep) {
    const uint32_t T = rowops::threshold(p, flags);
    for (int64_t l = 0; l < L; ++l)
        for (int64_t i = 0; i < N; ++i)
            for (int64_t k = 0; k < F; ++k) keep[(l * N + i) * F + k] = rowops::keep_of(seed, l, i, k, F, T) ? 1 : 0;
}

// y (L, N, F).  Returns 0, or 1 for arguments the library refuses.
int rowops_forward(const float* x, int64_t L, int64_t N, int64_t F, const float* b, const float* slope, double p, uint64_t seed, int flags,
                   float* y) {
    if (!rowops::args_ok(L, N, F, flags, slope != nullptr, p)) return 1;
    const uint32_t T = rowops::threshold(p, flags);
    const double s = rowops::scale(T);
    for (int64_t l = 0; l < L; ++l)
        for (int64_t i = 0; i < N; ++i)
            for (int64_t k = 0; k < F; ++k) {
                const int64_t e = (l * N + i) * F + k;
                y[e] = rowops::y_of(x[e], col_of(k, b, slope, flags), rowops::keep_of(seed, l, i, k, F, T), s, flags);
            }
    return 0;
}

// gx (L, N, F), gb (F), gs (1 or F); null ones are skipped
int rowops_backward(const float* x, const float* gy, int64_t L, int64_t N, int64_t F, const float* b, const float* slope, double p,
                    uint64_t seed, int flags, float* gx, float* gb, float* gs) {
    if (!rowops::args_ok(L, N, F, flags, slope != nullptr, p)) return 1;
    const uint32_t T = rowops::threshold(p, flags);
    const double s = rowops::scale(T);
    const bool prelu = (flags & rowops::ACT_PRELU) != 0;
    std::vector<double> sA((size_t)F, 0.0), sC((size_t)F, 0.0);
    for (int64_t l = 0; l < L; ++l) {
        const float* xl = x + l * N * F;
        const float* gl = gy + l * N * F;
        for (int64_t k = 0; k < F; ++k) {
            const rowops::Col c = col_of(k, b, slope, flags);
            const auto keep = [&](int64_t i) { return rowops::keep_of(seed, l, i, k, F, T); };
            const auto gv = [&](int64_t i) { return rowops::gv_of(xl[i * F + k], gl[i * F + k], c, keep(i), s, flags); };
            sA[k] = sA[k] + rule_sum(N, one, gv);
            if (prelu) sC[k] = sC[k] + rule_sum(N, one, [&](int64_t i) { return rowops::slope_term(xl[i * F + k], gl[i * F + k], c, keep(i), s); });
            if (gx)
                for (int64_t i = 0; i < N; ++i) gx[(l * N + i) * F + k] = (float)gv(i);
        }
    }
    for (int64_t k = 0; k < F; ++k) {
        if (gb) gb[k] = (float)sA[k];
        if (gs && prelu && (flags & rowops::SLOPE_PER_CHANNEL)) gs[k] = (float)sC[k];
    }
    if (gs && prelu && !(flags & rowops::SLOPE_PER_CHANNEL)) {
        double total = 0.0;
        for (int64_t k = 0; k < F; ++k) total = total + sC[k];
        gs[0] = (float)total;
    }
    return 0;
}

// ---- layer norm
int rowops_ln_args_ok(int64_t L, int64_t N, int64_t F, int flags, int has_slope, double p, double eps) {
    return rowops::ln_args_ok(L, N, F, flags, has_slope != 0, p, eps) ? 1 : 0;
}
int rowops_ln_lg(int64_t F) { return rowops::ln_lg(F); }
int rowops_ln_instance(int64_t F) { return rowops::ln_instance(F); }
int64_t rowops_ln_backward_bytes(int64_t L, int64_t N, int64_t F, int want_weight, int want_bias, int want_slope) {
    return rowops::ln_backward_bytes(L, N, F, rowops::ln_planes_of(want_weight != 0, want_bias != 0, want_slope != 0));
}
// the row sum of F float64 terms, in the rule's order
double rowops_row_sum(const double* terms, int64_t F) { return rowops::row_sum(F, [&](int64_t k) { return terms[k]; }); }

}  // extern "C"

namespace {

rowops::LnCol ln_col_of(int64_t k, const float* w, const float* b, const float* slope, int flags) {
    rowops::LnCol c{};
    c.w = w ? (double)w[k] : 1.0;
    c.b = b ? (double)b[k] : 0.0;
    c.a = (flags & rowops::ACT_PRELU) ? (double)slope[(flags & rowops::SLOPE_PER_CHANNEL) ? k : 0] : 0.0;
    return c;
}

rowops::Row row_of(const float* xr, int64_t F, double eps) {
    rowops::Row r{};
    r.mean = rowops::ln_mean(rowops::row_sum(F, [&](int64_t k) { return (double)xr[k]; }), F);
    const double var = rowops::ln_mean(rowops::row_sum(F, [&](int64_t k) { return rowops::ln_square(rowops::ln_centred(xr[k], r.mean)); }), F);
    r.rstd = rowops::ln_rstd(var, eps);
    return r;
}

}  // namespace

extern "C" {

// y (L, N, F); stat (L, N, 2) mean, rstd (nullable)
int rowops_ln_forward(const float* x, int64_t L, int64_t N, int64_t F, const float* w, const float* b, const float* slope, double eps, double p,
                      uint64_t seed, int flags, float* y, double* stat) {
    if (!rowops::ln_args_ok(L, N, F, flags, slope != nullptr, p, eps)) return 1;
    const uint32_t T = rowops::threshold(p, flags);
    const double s = rowops::scale(T);
    for (int64_t l = 0; l < L; ++l)
        for (int64_t i = 0; i < N; ++i) {
            const float* xr = x + (l * N + i) * F;
            const rowops::Row r = row_of(xr, F, eps);
            if (stat) { stat[2 * (l * N + i)] = r.mean; stat[2 * (l * N + i) + 1] = r.rstd; }
            for (int64_t k = 0; k < F; ++k)
                y[(l * N + i) * F + k] = rowops::ln_y(xr[k], r, ln_col_of(k, w, b, slope, flags), rowops::keep_of(seed, l, i, k, F, T), s, flags);
        }
    return 0;
}

// gx (L, N, F), gw (F), gb (F), gs (1 or F); null ones are skipped
int rowops_ln_backward(const float* x, const float* gy, int64_t L, int64_t N, int64_t F, const float* w, const float* b, const float* slope,
                       double eps, double p, uint64_t seed, int flags, float* gx, float* gw, float* gb, float* gs) {
    if (!rowops::ln_args_ok(L, N, F, flags, slope != nullptr, p, eps)) return 1;
    const uint32_t T = rowops::threshold(p, flags);
    const double s = rowops::scale(T);
    const bool prelu = (flags & rowops::ACT_PRELU) != 0;
    std::vector<double> sA((size_t)F, 0.0), sW((size_t)F, 0.0), sC((size_t)F, 0.0);
    std::vector<rowops::Row> rows((size_t)N);
    for (int64_t l = 0; l < L; ++l) {
        const float* xl = x + l * N * F;
        const float* gl = gy + l * N * F;
        for (int64_t i = 0; i < N; ++i) {
            const float* xr = xl + i * F;
            const float* gr = gl + i * F;
            const rowops::Row r = rows[(size_t)i] = row_of(xr, F, eps);
            if (!gx) continue;
            const auto g = [&](int64_t k) {
                const rowops::LnCol c = ln_col_of(k, w, b, slope, flags);
                return rowops::ln_g(rowops::ln_gv(xr[k], gr[k], r, c, rowops::keep_of(seed, l, i, k, F, T), s, flags), c);
            };
            const double mg = rowops::ln_mean(rowops::row_sum(F, g), F);
            const double mgx = rowops::ln_mean(rowops::row_sum(F, [&](int64_t k) { return rowops::ln_gxh(g(k), rowops::ln_xhat(xr[k], r)); }), F);
            for (int64_t k = 0; k < F; ++k) gx[(l * N + i) * F + k] = rowops::ln_gx(g(k), rowops::ln_xhat(xr[k], r), mg, mgx, r.rstd);
        }
        if (!gw && !gb && !gs) continue;
        for (int64_t k = 0; k < F; ++k) {
            const rowops::LnCol c = ln_col_of(k, w, b, slope, flags);
            const auto keep = [&](int64_t i) { return rowops::keep_of(seed, l, i, k, F, T); };
            const auto gv = [&](int64_t i) { return rowops::ln_gv(xl[i * F + k], gl[i * F + k], rows[(size_t)i], c, keep(i), s, flags); };
            const auto xh = [&](int64_t i) { return rowops::ln_xhat(xl[i * F + k], rows[(size_t)i]); };
            sA[k] = sA[k] + rule_sum(N, one, gv);
            sW[k] = sW[k] + rule_sum(N, gv, xh);
            if (prelu) sC[k] = sC[k] + rule_sum(N, one, [&](int64_t i) { return rowops::ln_slope_term(xl[i * F + k], gl[i * F + k], rows[(size_t)i], c, keep(i), s); });
        }
    }
    for (int64_t k = 0; k < F; ++k) {
        if (gb) gb[k] = (float)sA[k];
        if (gw) gw[k] = (float)sW[k];
        if (gs && prelu && (flags & rowops::SLOPE_PER_CHANNEL)) gs[k] = (float)sC[k];
    }
    if (gs && prelu && !(flags & rowops::SLOPE_PER_CHANNEL)) {
        double total = 0.0;
        for (int64_t k = 0; k < F; ++k) total = total + sC[k];
        gs[0] = (float)total;
    }
    return 0;
}

}  // extern "C"
