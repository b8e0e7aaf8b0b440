// Host mirror of the fused InfoNCE loss (tests/test_infonce_cpu.py, tests/test_gpu_infonce.py): every value comes from
// rlap_amd/csrc/rlap_infonce.h, compiled with g++ and contraction off, so that it computes the bits the kernels compute.  The loops
// below restate only the ORDER the header fixes: parts, tiles, registers, lane halves.  `block_rows` groups the owner rows the way a
// different tiling of them would (and deals them to threads); no result may depend on it.
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

#include "rlap_infonce.h"

using namespace rlap;

namespace {

// run body(i0, i1) over [0, N) in blocks of `block` rows, on up to `threads` threads
template <class Body>
void over_blocks(int64_t N, int64_t block, int threads, Body body) {
    const int64_t nb = (N + block - 1) / block;
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

// D[k] = the chain over the stream rows of prob(owner, stream row) * stream[row][k], in the header's order
template <class Prob>
void stream_chain(int64_t N, int64_t F, const float* stream, Prob prob, float* D) {
    std::vector<float> acc((size_t)F);
    for (int64_t k = 0; k < F; ++k) D[k] = 0.0f;
    for (int64_t p = 0; p < infonce::num_parts(N); ++p) {
        std::fill(acc.begin(), acc.end(), 0.0f);
        for (int64_t t = infonce::part_begin(N, p); t < infonce::part_begin(N, p + 1); ++t)
            for (int r = 0; r < 16; ++r)
                for (int h = 0; h < 2; ++h) {
                    const int64_t j = t * infonce::TILE + infonce::reg_row(r, h);
                    if (j < N) {
                        const float pj = prob(j);
                        for (int64_t k = 0; k < F; ++k) acc[k] = infonce::sim_step(acc[k], pj, stream[j * F + k]);
                    } else {
                        for (int64_t k = 0; k < F; ++k) acc[k] = infonce::sim_step(acc[k], 0.0f, 0.0f);
                    }
                }
        for (int64_t k = 0; k < F; ++k) D[k] = D[k] + acc[k];
    }
}

void push_through(int64_t F, double gs, double c, double itau, const float* own, const float* other, const float* D, double n2, float* out) {
    const bool clamped = infonce::norm_clamped(n2);
    const double nrm = infonce::norm_of(n2);
    double dot = 0.0;
    for (int64_t k = 0; k < F; ++k) dot = infonce::dot_step(dot, own[k], infonce::grad_hat(gs, c, other[k], itau, D[k]));
    for (int64_t k = 0; k < F; ++k) out[k] = infonce::grad_in(infonce::grad_hat(gs, c, other[k], itau, D[k]), own[k], dot, nrm, clamped);
}

}  // namespace

extern "C" {

float infonce_expw(float x) { return infonce::expw(x); }
void infonce_expw_many(const float* x, int64_t n, float* y) {
    for (int64_t i = 0; i < n; ++i) y[i] = infonce::expw(x[i]);
}
int64_t infonce_parts(int64_t N) { return infonce::num_parts(N); }
int64_t infonce_part_begin(int64_t N, int64_t p) { return infonce::part_begin(N, p); }
int infonce_reg_row(int r, int h) { return infonce::reg_row(r, h); }
int infonce_tau_ok(double tau) { return infonce::tau_ok(tau) ? 1 : 0; }
// the rule both launch_backward_main call, for the regime accounting of tests/test_gpu_loss_regimes.py
int infonce_feature_tiles(int64_t F) { return infonce::feature_tiles(F); }
int infonce_main_instance(int nft) { return infonce::main_instance(nft); }

// Z [N], rows [N], loss [1], sii [N]; ga, gb (N, F) when ga != nullptr (with the upstream gradient g).  Returns 0, or 1 for arguments
// the library refuses.
int infonce_mirror(const float* a, const float* b, int64_t N, int64_t F, double tau, int raw, int64_t block_rows, int threads, double g,
                   double* Z, double* rows, double* loss, float* sii, float* ga, float* gb) {
    if (N < 1 || F < 1 || F > infonce::MAX_F || !infonce::tau_ok(tau) || block_rows < 1) return 1;
    const Hats A = normalise(a, N, F), B = normalise(b, N, F);
    const float itf = infonce::inv_tau_f(tau);
    const double itau = infonce::inv_tau(tau), c = infonce::positive_coef(raw != 0, tau);
    std::vector<float> E((size_t)(N * N));   // e_ij, anchor-major
    over_blocks(N, block_rows, threads, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            for (int64_t j = 0; j < N; ++j) {
                const float s = similarity(B.h.data() + j * F, A.h.data() + i * F, F);   // (stream first, as the kernel's operands)
                if (j == i) sii[i] = s;
                E[i * N + j] = infonce::expw(infonce::exp_arg(s, itf));
            }
            double total = 0.0;
            for (int64_t p = 0; p < infonce::num_parts(N); ++p) {
                double half[2] = {0.0, 0.0};
                for (int64_t t = infonce::part_begin(N, p); t < infonce::part_begin(N, p + 1); ++t)
                    for (int h = 0; h < 2; ++h)
                        for (int r = 0; r < 16; ++r) {
                            const int64_t j = t * infonce::TILE + infonce::reg_row(r, h);
                            if (j < N) half[h] = half[h] + (double)E[i * N + j];
                        }
                total = total + (half[0] + half[1]);
            }
            Z[i] = total;
            rows[i] = infonce::row_term(c, sii[i], itau, total);
        }
    });
    *loss = infonce::loss_of(spmm::list_sum(N, [](int64_t) { return 1.0; }, [&](int64_t e) { return rows[e]; }, false, 0.0, 0.0), N);
    if (!ga) return 0;
    std::vector<float> rz((size_t)N);
    for (int64_t i = 0; i < N; ++i) rz[i] = infonce::recip_z(Z[i]);
    const double gs = infonce::grad_scale(g, N);
    over_blocks(N, block_rows, threads, [&](int64_t i0, int64_t i1) {
        std::vector<float> D((size_t)F);
        for (int64_t i = i0; i < i1; ++i) {
            // the anchor owns, the samples stream
            stream_chain(N, F, B.h.data(), [&](int64_t j) { return infonce::prob(E[i * N + j], rz[i]); }, D.data());
            push_through(F, gs, c, itau, A.h.data() + i * F, B.h.data() + i * F, D.data(), A.n2[i], ga + i * F);
            // the sample owns, the anchors stream
            stream_chain(N, F, A.h.data(), [&](int64_t j) { return infonce::prob(E[j * N + i], rz[j]); }, D.data());
            push_through(F, gs, c, itau, B.h.data() + i * F, A.h.data() + i * F, D.data(), B.n2[i], gb + i * F);
        }
    });
    return 0;
}

}  // extern "C"
