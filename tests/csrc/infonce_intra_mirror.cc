// Host mirror of the InfoNCE calls with intraview negatives (tests/test_infonce_intra_cpu.py, tests/test_gpu_infonce_intra.py): every
// value comes from rlap_amd/csrc/rlap_infonce.h, compiled with g++ and contraction off, so that it computes the bits the kernels
// compute.  The loops below restate only the ORDER the header fixes: for the row sums the parts, tiles, registers and lane halves of
// the one-direction rule (one-way) or the pair's parts, spans, groups and tree (pair), followed by the parts of the intraview sums;
// for the backward chains one accumulator a part, the part's tiles of the other view and then the same tiles of the own view.
// `block_rows` groups the owner rows the way a different tiling of them would (and deals them to threads); no result may depend on it.
#include <algorithm>
#include <cstdint>
#include <thread>
#include <vector>

#include "rlap_infonce.h"

using namespace rlap;

namespace {

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

// e of owner row i against every stream row j (the stream first, as the kernel's operands), and s_ii where sii != nullptr
void exp_row(const Hats& own, const Hats& str, int64_t N, int64_t F, float itf, int64_t i, float* e, float* sii) {
    for (int64_t j = 0; j < N; ++j) {
        const float s = similarity(str.h.data() + j * F, own.h.data() + i * F, F);
        if (sii && j == i) *sii = s;
        e[j] = infonce::expw(infonce::exp_arg(s, itf));
    }
}

// the sum of e[j] over the columns of the tiles [tb, te) that keep(j) admits: two float64 sums, one per lane half; half 0 + half 1
template <class Keep>
double tiles_sum(const float* e, int64_t N, int64_t tb, int64_t te, Keep keep) {
    double half[2] = {0.0, 0.0};
    for (int64_t t = tb; t < te; ++t)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) {
                const int64_t j = t * infonce::TILE + infonce::reg_row(r, h);
                if (j < N && keep(j)) half[h] = half[h] + (double)e[j];
            }
    return half[0] + half[1];
}

// total + the parts of the one-direction rule in order
template <class Keep>
double add_parts(double total, const float* e, int64_t N, Keep keep) {
    for (int64_t p = 0; p < infonce::num_parts(N); ++p) total = total + tiles_sum(e, N, infonce::part_begin(N, p), infonce::part_begin(N, p + 1), keep);
    return total;
}

// D[k]: one accumulator a part -- the part's tiles of `other` with the weight w_other(j), then the same tiles of `own` with the
// weight w_own(j), which is 0 for a row that is left out
template <class WOther, class WOwn>
void two_stream_chain(int64_t N, int64_t F, const float* other, const float* own, WOther w_other, WOwn w_own, float* D) {
    std::vector<float> acc((size_t)F);
    for (int64_t k = 0; k < F; ++k) D[k] = 0.0f;
    for (int64_t p = 0; p < infonce::num_parts(N); ++p) {
        std::fill(acc.begin(), acc.end(), 0.0f);
        for (int pass = 0; pass < 2; ++pass) {
            const float* stream = pass ? own : other;
            for (int64_t t = infonce::part_begin(N, p); t < infonce::part_begin(N, p + 1); ++t)
                for (int r = 0; r < 16; ++r)
                    for (int h = 0; h < 2; ++h) {
                        const int64_t j = t * infonce::TILE + infonce::reg_row(r, h);
                        const float wj = j < N ? (pass ? w_own(j) : w_other(j)) : 0.0f;
                        for (int64_t k = 0; k < F; ++k) acc[k] = infonce::sim_step(acc[k], wj, j < N ? stream[j * F + k] : 0.0f);
                    }
        }
        for (int64_t k = 0; k < F; ++k) D[k] = D[k] + acc[k];
    }
}

// the one-direction rule's chain over one stream (the sample-owner chain of the one-way call)
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

void push_through(int64_t F, double gs, double c, double itau, const float* own, const float* other, const float* D, double n2, float* out) {
    const bool clamped = infonce::norm_clamped(n2);
    const double nrm = infonce::norm_of(n2);
    double dot = 0.0;
    for (int64_t k = 0; k < F; ++k) dot = infonce::dot_step(dot, own[k], infonce::grad_hat(gs, c, other[k], itau, D[k]));
    for (int64_t k = 0; k < F; ++k) out[k] = infonce::grad_in(infonce::grad_hat(gs, c, other[k], itau, D[k]), own[k], dot, nrm, clamped);
}

}  // namespace

extern "C" {

int intra_ok(int intraview) { return infonce::intra_ok(intraview) ? 1 : 0; }
int intra_member(int intraview, int64_t i, int64_t j) { return infonce::intra_member(intraview, i, j) ? 1 : 0; }
int64_t intra_z_parts(int64_t N) { return infonce::intra_z_parts(N); }

// One-way.  Z [N], rows [N], loss [1], sii [N]; ga, gb (N, F) when ga != nullptr (with the upstream gradient g).  Returns 0, or 1 for
// arguments the library refuses.
int infonce_intra_mirror(const float* a, const float* b, int64_t N, int64_t F, double tau, int raw, int intraview, int64_t block_rows, int threads,
                         double g, double* Z, double* rows, double* loss, float* sii, float* ga, float* gb) {
    if (N < 1 || F < 1 || F > infonce::MAX_F || !infonce::tau_ok(tau) || !infonce::intra_ok(intraview) || block_rows < 1) return 1;
    const Hats A = normalise(a, N, F), B = normalise(b, N, F);
    const float itf = infonce::inv_tau_f(tau);
    const double itau = infonce::inv_tau(tau), c = infonce::positive_coef(raw != 0, tau);
    std::vector<float> E((size_t)(N * N)), EA((size_t)(N * N));   // e^ab_ij and e^aa_ij, anchor-major
    over_blocks(N, block_rows, threads, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            exp_row(A, B, N, F, itf, i, E.data() + i * N, sii + i);
            exp_row(A, A, N, F, itf, i, EA.data() + i * N, nullptr);
            double total = add_parts(0.0, E.data() + i * N, N, [](int64_t) { return true; });
            total = add_parts(total, EA.data() + i * N, N, [&](int64_t j) { return infonce::intra_member(intraview, i, j); });
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
            // the anchor owns: the samples stream, then the anchors
            two_stream_chain(N, F, B.h.data(), A.h.data(), [&](int64_t j) { return infonce::prob(E[i * N + j], rz[i]); },
                             [&](int64_t j) { return infonce::intra_member(intraview, i, j) ? infonce::pair_weight(EA[i * N + j], rz[i], rz[j]) : 0.0f; }, D.data());
            push_through(F, gs, c, itau, A.h.data() + i * F, B.h.data() + i * F, D.data(), A.n2[i], ga + i * F);
            // the sample owns, the anchors stream
            stream_chain(N, F, A.h.data(), [&](int64_t j) { return infonce::prob(E[j * N + i], rz[j]); }, D.data());
            push_through(F, gs, c, itau, B.h.data() + i * F, A.h.data() + i * F, D.data(), B.n2[i], gb + i * F);
        }
    });
    return 0;
}

// The pair.  Z [2, N] (Z, then Zc), rows [2, N], loss [1], sii [N]; ga, gb as above.
int infonce_pair_intra_mirror(const float* a, const float* b, int64_t N, int64_t F, double tau, int raw, int intraview, int64_t block_rows,
                              int threads, double g, double* Z, double* rows, double* loss, float* sii, float* ga, float* gb) {
    if (N < 1 || F < 1 || F > infonce::MAX_F || !infonce::tau_ok(tau) || !infonce::intra_ok(intraview) || block_rows < 1) return 1;
    const Hats A = normalise(a, N, F), B = normalise(b, N, F);
    const float itf = infonce::inv_tau_f(tau);
    const double itau = infonce::inv_tau(tau), c = infonce::positive_coef(raw != 0, tau);
    const int64_t T = infonce::num_tiles(N);
    double* Zc = Z + N;
    std::vector<float> E((size_t)(N * N)), EA((size_t)(N * N)), EB((size_t)(N * N));   // e^ab_ij anchor-major, e^aa, e^bb
    over_blocks(N, block_rows, threads, [&](int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) {
            exp_row(A, B, N, F, itf, i, E.data() + i * N, sii + i);
            exp_row(A, A, N, F, itf, i, EA.data() + i * N, nullptr);
            exp_row(B, B, N, F, itf, i, EB.data() + i * N, nullptr);
            double total = 0.0;
            for (int64_t p = 0; p < infonce::pair_parts(N); ++p) {
                const int64_t tb = infonce::pair_part_begin(N, p), te = infonce::pair_part_begin(N, p + 1);
                double part = 0.0;
                for (int64_t sb = tb; sb < te; sb += infonce::PAIR_SPAN_TILES)
                    part = part + tiles_sum(E.data() + i * N, N, sb, std::min(te, sb + infonce::PAIR_SPAN_TILES), [](int64_t) { return true; });
                total = total + part;
            }
            total = add_parts(total, EA.data() + i * N, N, [&](int64_t j) { return infonce::intra_member(intraview, i, j); });
            Z[i] = total;
            rows[i] = infonce::row_term(c, sii[i], itau, total);
        }
    });
    over_blocks(N, block_rows, threads, [&](int64_t j0, int64_t j1) {
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
            total = add_parts(total, EB.data() + j * N, N, [&](int64_t i) { return infonce::intra_member(intraview, j, i); });
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
    over_blocks(N, block_rows, threads, [&](int64_t i0, int64_t i1) {
        std::vector<float> D((size_t)F);
        for (int64_t i = i0; i < i1; ++i) {
            two_stream_chain(N, F, B.h.data(), A.h.data(), [&](int64_t j) { return infonce::pair_weight(E[i * N + j], rza[i], rzb[j]); },
                             [&](int64_t j) { return infonce::intra_member(intraview, i, j) ? infonce::pair_weight(EA[i * N + j], rza[i], rza[j]) : 0.0f; }, D.data());
            push_through(F, gs2, c2, itau, A.h.data() + i * F, B.h.data() + i * F, D.data(), A.n2[i], ga + i * F);
            two_stream_chain(N, F, A.h.data(), B.h.data(), [&](int64_t j) { return infonce::pair_weight(E[j * N + i], rzb[i], rza[j]); },
                             [&](int64_t j) { return infonce::intra_member(intraview, i, j) ? infonce::pair_weight(EB[i * N + j], rzb[i], rzb[j]) : 0.0f; }, D.data());
            push_through(F, gs2, c2, itau, B.h.data() + i * F, A.h.data() + i * F, D.data(), B.n2[i], gb + i * F);
        }
    });
    return 0;
}

}  // extern "C"
