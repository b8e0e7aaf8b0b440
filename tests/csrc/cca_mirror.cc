// Host mirror of the fused CCA-SSG loss (tests/test_cca_cpu.py, tests/test_gpu_cca.py): every value comes from
// rlap_amd/csrc/rlap_cca.h, compiled with g++ and contraction off, so that it computes the bits the kernels compute.  The loops below
// restate only the ORDER the header fixes: chunks, parts, rows, columns.  `block` groups the columns (forward) and the rows
// (backward) the way a different tiling of them would and deals them to threads; `pad_tiles` appends that many 32-column tiles of
// zeros behind the padded image.  No result may depend on either.
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

#include "rlap_cca.h"

using namespace rlap;

namespace {

// run body(i0, i1) over [0, n) in blocks of `block`, on up to `threads` threads
template <class Body>
void over_blocks(int64_t n, int64_t block, int threads, Body body) {
    const int64_t nb = (n + block - 1) / block;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads, nb));
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; ++w)
        pool.emplace_back([=] {
            for (int64_t b = w; b < nb; b += nt) body(b * block, std::min(n, (b + 1) * block));
        });
    for (auto& t : pool) t.join();
}

const auto one = [](int64_t) { return 1.0; };

struct View {
    std::vector<float> z;   // N x F
};

// mean | sd of a view into stat[0 .. 2 F), the standardised copy
View standardise(const float* h, int64_t N, int64_t F, double* stat) {
    View v;
    v.z.resize((size_t)(N * F));
    for (int64_t k = 0; k < F; ++k) {
        const double mean = cca::col_mean(cca::rule_sum(N, one, [&](int64_t i) { return (double)h[i * F + k]; }), N);
        const auto d = [&](int64_t i) { return cca::centred(h[i * F + k], mean); };
        const double sd = cca::col_sd(cca::rule_sum(N, d, d), N);
        stat[k] = mean;
        stat[F + k] = sd;
        for (int64_t i = 0; i < N; ++i) v.z[i * F + k] = cca::zval(h[i * F + k], mean, sd);
    }
    return v;
}

// S_kl: the parts in order, each a chain over its rows, the rows behind N as fmaf(0, 0, acc)
double gram_sum(const float* z, int64_t N, int64_t F, int64_t k, int64_t l) {
    double S = 0.0;
    for (int64_t p = 0; p < cca::num_parts(N, F); ++p) {
        float acc = 0.0f;
        for (int64_t i = cca::part_begin(N, F, p); i < cca::part_begin(N, F, p + 1); ++i)
            acc = i < N ? cca::gram_step(acc, z[i * F + k], z[i * F + l]) : cca::gram_step(acc, 0.0f, 0.0f);
        S = S + (double)acc;
    }
    return S;
}

}  // namespace

extern "C" {

int64_t cca_parts(int64_t N, int64_t F) { return cca::num_parts(N, F); }
int64_t cca_part_begin(int64_t N, int64_t F, int64_t p) { return cca::part_begin(N, F, p); }
int64_t cca_pair_groups(int64_t F) { return cca::pair_groups(F); }
int cca_lambd_ok(double l) { return cca::lambd_ok(l) ? 1 : 0; }
// the rules both launchers call, for the regime accounting of tests/test_gpu_loss_regimes.py
int cca_feature_tiles(int64_t F) { return cca::feature_tiles(F); }
int cca_super_pairs(int64_t F) { return cca::super_pairs(F); }
int cca_gram_instance(int nft) { return cca::gram_instance(nft); }
int cca_zr_instance(int nft) { return cca::zr_instance(nft); }

// terms [4], colstat [4 F], gram [2 F F]; ga, gb (N, F) when ga != nullptr (with the upstream gradient g).  Returns 0, or 1 for
// arguments the library refuses.
int cca_mirror(const float* a, const float* b, int64_t N, int64_t F, double lambd, int64_t block, int threads, int pad_tiles, double g,
               double* terms, double* colstat, float* gram, float* ga, float* gb) {
    if (N < 2 || F < 1 || F > cca::MAX_F || !cca::lambd_ok(lambd) || block < 1 || pad_tiles < 0) return 1;
    const float* h[2] = {a, b};
    View V[2];
    for (int v = 0; v < 2; ++v) V[v] = standardise(h[v], N, F, colstat + v * 2 * F);
    const int64_t ff = F * F;
    std::vector<double> R((size_t)(2 * ff));
    for (int v = 0; v < 2; ++v) {
        const float* z = V[v].z.data();
        double* Rv = R.data() + v * ff;
        over_blocks(F, block, threads, [&](int64_t k0, int64_t k1) {
            for (int64_t k = k0; k < k1; ++k)
                for (int64_t l = k; l < F; ++l) {
                    const double r = cca::resid(gram_sum(z, N, F, k, l), N, k == l);
                    Rv[k * F + l] = r;
                    Rv[l * F + k] = r;
                }
        });
        for (int64_t e = 0; e < ff; ++e) gram[v * ff + e] = (float)Rv[e];
    }
    double dec[2];
    for (int v = 0; v < 2; ++v) {
        const double* Rv = R.data() + v * ff;
        const auto r = [&](int64_t e) { return Rv[e]; };
        dec[v] = cca::rule_sum(ff, r, r);
    }
    std::vector<double> d((size_t)F);
    for (int64_t k = 0; k < F; ++k)
        d[k] = cca::rule_sum(N, [&](int64_t i) { return (double)V[0].z[i * F + k]; }, [&](int64_t i) { return (double)V[1].z[i * F + k]; });
    const double inv = cca::inv_of(cca::rule_sum(F, one, [&](int64_t k) { return d[k]; }), N);
    terms[0] = cca::loss_of(inv, lambd, dec[0], dec[1]);
    terms[1] = inv;
    terms[2] = dec[0];
    terms[3] = dec[1];
    if (!ga) return 0;

    const int64_t Fchain = cca::padded_features(F) + (int64_t)pad_tiles * cca::TILE;
    const double c4 = cca::coef4(lambd, N);
    float* out[2] = {ga, gb};
    for (int v = 0; v < 2; ++v) {
        const float* z = V[v].z.data();
        const float* zo = V[1 - v].z.data();
        const float* r = gram + v * ff;
        std::vector<float> P((size_t)(N * F));
        over_blocks(N, block, threads, [&](int64_t i0, int64_t i1) {
            for (int64_t i = i0; i < i1; ++i)
                for (int64_t k = 0; k < F; ++k) {
                    float acc = 0.0f;
                    for (int64_t l = 0; l < Fchain; ++l)
                        acc = l < F ? cca::gram_step(acc, z[i * F + l], r[l * F + k]) : cca::gram_step(acc, 0.0f, 0.0f);
                    P[i * F + k] = acc;
                }
        });
        const double* stat = colstat + v * 2 * F;
        for (int64_t k = 0; k < F; ++k) {
            const auto dz = [&](int64_t i) { return cca::dz_of(g, zo[i * F + k], P[i * F + k], N, c4); };
            const double m = cca::col_m(cca::rule_sum(N, one, dz), N);
            const double q = cca::col_q(cca::rule_sum(N, dz, [&](int64_t i) { return (double)z[i * F + k]; }), N);
            for (int64_t i = 0; i < N; ++i) out[v][i * F + k] = cca::dh_of(dz(i), m, z[i * F + k], q, stat[F + k]);
        }
    }
    return 0;
}

}  // extern "C"
