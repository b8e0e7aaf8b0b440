// Host mirror of the fused dense layer (tests/test_linear_cpu.py, tests/test_gpu_linear.py): every value comes from
// rlap_amd/csrc/rlap_linear.h, compiled with g++ and contraction off, so that it computes the bits the kernels compute.  The loops
// below restate only the ORDER the header fixes: inner index, parts, rows, chunks.  Rows (forward, gx) and columns (gW, gb) are dealt
// to threads; no result may depend on how.
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

#include "rlap_linear.h"

using namespace rlap;

namespace {

// run body(i) for i in [0, n) on up to `threads` threads
template <class Body>
void over(int64_t n, int threads, Body body) {
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads, n));
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; ++w)
        pool.emplace_back([=] {
            for (int64_t i = w; i < n; i += nt) body(i);
        });
    for (auto& t : pool) t.join();
}

bool args_ok(int64_t M, int64_t Fin, int64_t Fout, int act, double alpha, int flags) {
    return linear::rows_ok(M) && linear::features_ok(Fin) && linear::features_ok(Fout) && linear::act_ok(act) && linear::alpha_ok(alpha) &&
           linear::flags_ok(flags);
}

}  // namespace

extern "C" {

int64_t lin_num_parts(int64_t M, int64_t Fin, int64_t Fout) { return linear::num_parts(M, Fin, Fout); }
int64_t lin_part_begin(int64_t M, int64_t Fin, int64_t Fout, int64_t p) { return linear::part_begin(M, Fin, Fout, p); }
int lin_feature_tiles(int64_t F) { return linear::feature_tiles(F); }
int lin_col_waves(int nct) { return linear::col_waves(nct); }
int lin_row_tiles(int nct) { return linear::row_tiles(nct); }
int lin_product_instance(int nct) { return linear::product_instance(nct); }
int64_t lin_product_groups(int64_t M, int nct) { return linear::product_groups(M, nct); }
int64_t lin_wave_row_tile(int64_t g, int w, int nct) { return linear::wave_row_tile(g, w, nct); }
int lin_wave_col_tile(int w, int j, int nct) { return linear::wave_col_tile(w, j, nct); }
int lin_super_tiles(int64_t F) { return linear::super_tiles(F); }
int lin_row_groups(int64_t Fout) { return linear::row_groups(Fout); }
int lin_pair_groups(int64_t Fin, int64_t Fout) { return linear::pair_groups(Fin, Fout); }
int lin_cross_instance(int nft) { return linear::cross_instance(nft); }
int lin_flags_ok(int flags) { return linear::flags_ok(flags) ? 1 : 0; }
int lin_act_ok(int act) { return linear::act_ok(act) ? 1 : 0; }
int lin_alpha_ok(double a) { return linear::alpha_ok(a) ? 1 : 0; }
int lin_vec_ok(int64_t F, uint64_t bits) { return linear::vec_ok(F, bits) ? 1 : 0; }

// y (M, Fout); b may be null.  pad_tiles appends that many 32-column tiles of zeros behind the padded inner index.  Returns 0, or 1
// for arguments the library refuses.
int lin_mirror(const float* x, const float* w, const float* b, int64_t M, int64_t Fin, int64_t Fout, int act, double alpha, int flags,
               int threads, int pad_tiles, float* y) {
    if (!args_ok(M, Fin, Fout, act, alpha, flags) || pad_tiles < 0) return 1;
    const int64_t K = linear::padded_features(Fin) + (int64_t)pad_tiles * linear::TILE;
    std::vector<float> wk((size_t)(Fin * Fout));               // W as (Fin, Fout), whatever the layout
    for (int64_t k = 0; k < Fin; ++k)
        for (int64_t o = 0; o < Fout; ++o) wk[k * Fout + o] = w[linear::weight_index(k, o, Fin, Fout, flags)];
    over(M, threads, [&](int64_t i) {
        for (int64_t o = 0; o < Fout; ++o) {
            float acc = 0.0f;
            for (int64_t k = 0; k < K; ++k) acc = k < Fin ? linear::chain_step(acc, x[i * Fin + k], wk[k * Fout + o]) : linear::chain_step(acc, 0.0f, 0.0f);
            y[i * Fout + o] = linear::y_of(acc, b != nullptr, b ? b[o] : 0.0f, act, alpha);
        }
    });
    return 0;
}

// gx (M, Fin), gw of w's layout, gb (Fout,): each may be null
int lin_mirror_backward(const float* x, const float* w, const float* y, const float* gy, int64_t M, int64_t Fin, int64_t Fout, int act,
                        double alpha, int flags, int threads, int pad_tiles, float* gx, float* gw, float* gb) {
    if (!args_ok(M, Fin, Fout, act, alpha, flags) || pad_tiles < 0) return 1;
    std::vector<float> t((size_t)(M * Fout));                  // (the mirror may keep t: the values are what counts)
    for (int64_t e = 0; e < M * Fout; ++e) t[e] = linear::t_of(gy[e], y[e], act, alpha);
    if (gx) {
        const int64_t C = linear::padded_features(Fout) + (int64_t)pad_tiles * linear::TILE;
        over(M, threads, [&](int64_t i) {
            for (int64_t k = 0; k < Fin; ++k) {
                float acc = 0.0f;
                for (int64_t o = 0; o < C; ++o)
                    acc = o < Fout ? linear::chain_step(acc, t[i * Fout + o], w[linear::weight_index(k, o, Fin, Fout, flags)])
                                   : linear::chain_step(acc, 0.0f, 0.0f);
                gx[i * Fin + k] = acc;
            }
        });
    }
    if (gw) {
        const int64_t P = linear::num_parts(M, Fin, Fout);
        over(Fin, threads, [&](int64_t k) {
            for (int64_t o = 0; o < Fout; ++o) {
                double S = 0.0;
                for (int64_t p = 0; p < P; ++p) {
                    float acc = 0.0f;
                    for (int64_t i = linear::part_begin(M, Fin, Fout, p); i < linear::part_begin(M, Fin, Fout, p + 1); ++i)
                        acc = i < M ? linear::chain_step(acc, x[i * Fin + k], t[i * Fout + o]) : linear::chain_step(acc, 0.0f, 0.0f);
                    S = S + (double)acc;
                }
                gw[linear::weight_index(k, o, Fin, Fout, flags)] = (float)S;
            }
        });
    }
    if (gb) {
        over(Fout, threads, [&](int64_t o) {
            gb[o] = (float)linear::rule_sum(M, [](int64_t) { return 1.0; }, [&](int64_t i) { return (double)t[i * Fout + o]; });
        });
    }
    return 0;
}

}  // extern "C"
