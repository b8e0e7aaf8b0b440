// Host mirror of the symmetric InfoNCE pair (tests/test_infonce_pair_cpu.py, tests/test_gpu_infonce_pair.py): every value comes from
// rlap_amd/csrc/rlap_infonce.h, compiled with g++ and contraction off, so that it computes the bits the kernels compute.  The loops
// below restate only the ORDER the header fixes: for Z the parts, spans, tiles, registers and lane halves; for Zc the groups, row
// blocks, owner tiles and the tree over a tile's rows; for the backward chains the parts, tiles, registers and halves of the
// one-direction rule with the pair's weight.
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

#include "rlap_infonce.h"

using namespace rlap;

namespace {

template <class Body>
void over_rows(int64_t N, int threads, Body body) {
    const int64_t block = 32, nb = (N + block - 1) / block;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(threads, nb));
    std::vector<std::thread> pool;
    for (int w = 0; w < nt; ++w)
        pool.emplace_back([=] {
            for (int64_t b = w; b < nb; b += nt) body(b * block, std::min(N, (b + 1) * block));
        });
    for (auto& t : pool) t.join();
}

struct Hats {
    std::vector<float> h;
    std::vector<double> n2;
};

Hats normalise(const float* x, int64_t N, int64_t F) {
    Hats out;
    out.h.resize((size_t)(N * F));
    out.n2.resize((size_t)N);
    for (int64_t i = 0; i < N; ++i) {
        out.n2[i] = infonce::norm2(x + i * F, F);
        const double nrm = infonce::norm_of(out.n2[i]);
        for (int64_t k = 0; k < F; ++k) out.h[i * F + k] = infonce::hat(x[i * F + k], nrm);
    }
    return out;
}

float similarity(const float* x, const float* y, int64_t F) {
    float acc = 0.0f;
    for (int64_t k = 0; k < F; ++k) acc = infonce::sim_step(acc, x[k], y[k]);
    return acc;
}

// D[k] = the chain over the stream rows of weight(stream row) * stream[row][k]: the one-direction rule's parts and order
template <class Weight>
void stream_chain(int64_t N, int64_t F, const float* stream, Weight weight, float* D) {
    std::vector<float> acc((size_t)F);
    for (int64_t k = 0; k < F; ++k) D[k] = 0.0f;
    for (int64_t p = 0; p < infonce::num_parts(N); ++p) {
        std::fill(acc.begin(), acc.end(), 0.0f);
        for (int64_t t = infonce::part_begin(N, p); t < infonce::part_begin(N, p + 1); ++t)
            for (int r = 0; r < 16; ++r)
                for (int h = 0; h < 2; ++h) {
                    const int64_t j = t * infonce::TILE + infonce::reg_row(r, h);
                    const float wj = j < N ? weight(j) : 0.0f;
                    for (int64_t k = 0; k < F; ++k) acc[k] = infonce::sim_step(acc[k], wj, j < N ? stream[j * F + k] : 0.0f);
                }
        for (int64_t k = 0; k < F; ++k) D[k] = D[k] + acc[k];
    }
}

void push_through(int64_t F, double gs2, double c2, double itau, const float* own, const float* other, const float* D, double n2, float* out) {
    const bool clamped = infonce::norm_clamped(n2);
    const double nrm = infonce::norm_of(n2);
    double dot = 0.0;
    for (int64_t k = 0; k < F; ++k) dot = infonce::dot_step(dot, own[k], infonce::grad_hat(gs2, c2, other[k], itau, D[k]));
    for (int64_t k = 0; k < F; ++k) out[k] = infonce::grad_in(infonce::grad_hat(gs2, c2, other[k], itau, D[k]), own[k], dot, nrm, clamped);
}

}  // namespace

extern "C" {

int64_t pair_groups(int64_t N) { return infonce::pair_groups(N); }
int64_t pair_group_begin(int64_t N, int64_t g) { return infonce::pair_group_begin(N, g); }
int64_t pair_parts(int64_t N) { return infonce::pair_parts(N); }
int64_t pair_part_begin(int64_t N, int64_t p) { return infonce::pair_part_begin(N, p); }
int64_t pair_span_tiles(int64_t N) { return infonce::pair_span_tiles(N); }
int64_t pair_span_cap(void) { return infonce::PAIR_SPAN_TILES; }
double pair_tree32(const double* x) { return infonce::tree32(x); }

// Z [2, N] (Z, then Zc), rows [2, N], loss [1], sii [N]; ga, gb (N, F) when ga != nullptr (with the upstream gradient g).  Returns 0,
// or 1 for arguments the library refuses.
int infonce_pair_mirror(const float* a, const float* b, int64_t N, int64_t F, double tau, int raw, int threads, double g, double* Z,
                        double* rows, double* loss, float* sii, float* ga, float* gb) {
    if (N < 1 || F < 1 || F > infonce::MAX_F || !infonce::tau_ok(tau)) return 1;
    const Hats A = normalise(a, N, F), B = normalise(b, N, F);
    const float itf = infonce::inv_tau_f(tau);
    const double itau = infonce::inv_tau(tau), c = infonce::positive_coef(raw != 0, tau);
    const int64_t T = infonce::num_tiles(N);
    double* Zc = Z + N;
    std::vector<float> E((size_t)(N * N));   // e_ij, anchor-major
    over_rows(N, threads, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            for (int64_t j = 0; j < N; ++j) {
                const float s = similarity(B.h.data() + j * F, A.h.data() + i * F, F);   // (stream first, as the kernel's operands)
                if (j == i) sii[i] = s;
                E[i * N + j] = infonce::expw(infonce::exp_arg(s, itf));
            }
            double total = 0.0;
            for (int64_t p = 0; p < infonce::pair_parts(N); ++p) {
                const int64_t tb = infonce::pair_part_begin(N, p), te = infonce::pair_part_begin(N, p + 1);
                double part = 0.0;
                for (int64_t sb = tb; sb < te; sb += infonce::PAIR_SPAN_TILES) {
                    const int64_t se = std::min(te, sb + infonce::PAIR_SPAN_TILES);
                    double half[2] = {0.0, 0.0};
                    for (int64_t t = sb; t < se; ++t)
                        for (int h = 0; h < 2; ++h)
                            for (int r = 0; r < 16; ++r) {
                                const int64_t j = t * infonce::TILE + infonce::reg_row(r, h);
                                if (j < N) half[h] = half[h] + (double)E[i * N + j];
                            }
                    part = part + (half[0] + half[1]);
                }
                total = total + part;
            }
            Z[i] = total;
            rows[i] = infonce::row_term(c, sii[i], itau, total);
        }
    });
    over_rows(N, threads, [&](int64_t j0, int64_t j1) {
        for (int64_t j = j0; j < j1; ++j) {
            double total = 0.0;
            for (int64_t q = 0; q < infonce::pair_groups(N); ++q) {
                double group = 0.0;
                for (int64_t blk = infonce::pair_group_begin(N, q); blk < infonce::pair_group_begin(N, q + 1); ++blk)
                    for (int wave = 0; wave < infonce::BLOCK_TILES; ++wave) {
                        const int64_t ot = blk * infonce::BLOCK_TILES + wave;
                        double v[infonce::TILE];
                        for (int cc = 0; cc < infonce::TILE; ++cc) {
                            const int64_t i = ot * infonce::TILE + cc;
                            v[cc] = ot < T && i < N ? (double)E[i * N + j] : 0.0;
                        }
                        group = group + infonce::tree32(v);
                    }
                total = total + group;
            }
            Zc[j] = total;
            rows[N + j] = infonce::row_term(c, sii[j], itau, total);
        }
    });
    const double ta = spmm::list_sum(N, [](int64_t) { return 1.0; }, [&](int64_t e) { return rows[e]; }, false, 0.0, 0.0);
    const double tb = spmm::list_sum(N, [](int64_t) { return 1.0; }, [&](int64_t e) { return rows[N + e]; }, false, 0.0, 0.0);
    *loss = infonce::pair_loss_of(ta, tb, N);
    if (!ga) return 0;
    std::vector<float> rza((size_t)N), rzb((size_t)N);
    for (int64_t i = 0; i < N; ++i) { rza[i] = infonce::recip_z(Z[i]); rzb[i] = infonce::recip_z(Zc[i]); }
    const double gs2 = infonce::pair_grad_scale(g, N), c2 = infonce::pair_positive_coef(raw != 0, tau);
    over_rows(N, threads, [&](int64_t i0, int64_t i1) {
        std::vector<float> D((size_t)F);
        for (int64_t i = i0; i < i1; ++i) {
            // the anchor owns, the samples stream
            stream_chain(N, F, B.h.data(), [&](int64_t j) { return infonce::pair_weight(E[i * N + j], rza[i], rzb[j]); }, D.data());
            push_through(F, gs2, c2, itau, A.h.data() + i * F, B.h.data() + i * F, D.data(), A.n2[i], ga + i * F);
            // the sample owns, the anchors stream
            stream_chain(N, F, A.h.data(), [&](int64_t j) { return infonce::pair_weight(E[j * N + i], rzb[i], rza[j]); }, D.data());
            push_through(F, gs2, c2, itau, B.h.data() + i * F, A.h.data() + i * F, D.data(), B.n2[i], gb + i * F);
        }
    });
    return 0;
}

}  // extern "C"
