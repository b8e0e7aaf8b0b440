// The host-side arithmetic of the per-view batch norm (rlap_amd/csrc/rlap_norm.h: the refusals, the dispatch, the map from work item
// and lane to (layer, chunk, columns), the arena's size) and the mirror's loops (tests/csrc/norm_mirror.cc) in a stand-alone program,
// built with g++ -fsanitize=address,undefined by tests/test_norm_cpu.py.  usage: norm_main <largest N>.  Every (L, N, F, alignment)
// with L in {1, 3}, N up to the argument and F up to 70 (and a few wide ones) is checked exhaustively: every (layer, chunk, column)
// belongs to exactly one lane of one item, with the chunk's rows.  Prints "<n> sizes, <f> failures".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "norm_mirror.cc"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void check_map(int64_t L, int64_t N, int64_t F, bool aligned) {
    const readout::Dispatch d = norm::dispatch(F, aligned);
    const int64_t V = d.vec ? 4 : 1, nch = spmm::num_chunks(N), items = norm::num_items(L, N, d);
    CHECK(d.vec == (aligned && F % 4 == 0));
    CHECK(d.lanes * V == F && d.lg >= 0 && d.lg <= 6 && d.ftiles >= 1);
    CHECK(items == L * ((nch + (64 >> d.lg) - 1) / (64 >> d.lg)) * d.ftiles);
    const int sp = norm::apply_split(items);
    CHECK(sp >= 0 && sp <= 4 && (sp == 0 || (items << (sp - 1)) < norm::APPLY_WAVES) && (sp == 4 || (items << sp) >= norm::APPLY_WAVES));
    std::vector<int> seen((size_t)(L * nch * F), 0);
    norm::Item it{};
    CHECK(!norm::item_of(-1, 0, L, N, F, d, &it) && !norm::item_of(items, 0, L, N, F, d, &it) && !norm::item_of(0, 64, L, N, F, d, &it));
    for (int64_t w = 0; w < items; ++w)
        for (int lane = 0; lane < 64; ++lane) {
            if (!norm::item_of(w, lane, L, N, F, d, &it)) continue;
            bool ok = it.l >= 0 && it.l < L && it.q >= 0 && it.q < nch && it.f0 >= 0 && it.f0 + V <= F;
            ok = ok && it.r0 == it.q * spmm::CHUNK && it.r1 == (it.r0 + spmm::CHUNK < N ? it.r0 + spmm::CHUNK : N) && it.r0 < it.r1;
            if (!ok) { ++failures; std::printf("FAILED item L=%lld N=%lld F=%lld w=%lld lane=%d\n", (long long)L, (long long)N, (long long)F, (long long)w, lane); continue; }
            for (int64_t v = 0; v < V; ++v) ++seen[(size_t)((it.l * nch + it.q) * F + it.f0 + v)];
            if (lane == 0 && w % 7 == 0)   // the row ranges of the apply passes tile the item's rows, in order, whatever the split
                for (int s = 0; s <= 4; ++s) {
                    int64_t at = it.r0, a0, a1;
                    for (int64_t p = 0; p < (1 << s); ++p) {
                        norm::split_rows(it, s, p, &a0, &a1);
                        if (a0 < a1) { CHECK(a0 == at && a1 <= it.r1 && a1 - a0 <= (spmm::CHUNK >> s)); at = a1; }
                    }
                    CHECK(at == it.r1);
                }
        }
    for (int s : seen) if (s != 1) { ++failures; std::printf("FAILED cover L=%lld N=%lld F=%lld aligned=%d\n", (long long)L, (long long)N, (long long)F, (int)aligned); break; }
    for (int flags : {0, (int)norm::POST_PRELU, (int)norm::EVAL}) {
        const int64_t fb = norm::forward_bytes(L, N, F, flags), bb = norm::backward_bytes(L, N, F, flags);
        CHECK(fb % 256 == 0 && bb % 256 == 0);
        CHECK((flags & norm::EVAL) ? fb == 0 : fb >= (2 * L * nch * F + 2 * L * F) * 8);
        CHECK(bb >= (norm::backward_sums(flags) * L * nch * F + 5 * L * F) * 8);
    }
}

static void check_refusals() {
    const double nan = std::nan(""), inf = INFINITY;
    CHECK(norm::args_ok(1, 2, 1, 0, false, false, 1e-5, 0.1) && norm::args_ok(3, 2, 4096, norm::PRE_RELU | norm::POST_RELU, false, false, 1e-5, 0.0));
    CHECK(norm::args_ok(1, 1, 1, norm::EVAL, false, true, 1e-5, 1.0) && norm::args_ok(1, 2, 8, norm::POST_PRELU | norm::SLOPE_PER_CHANNEL, true, false, 1.0, 1.0));
    CHECK(!norm::args_ok(1, 2, 1, norm::POST_RELU | norm::POST_PRELU, true, false, 1e-5, 0.1));   // both post flags
    CHECK(!norm::args_ok(1, 2, 1, norm::POST_PRELU, false, false, 1e-5, 0.1));                   // PReLU without a slope
    CHECK(!norm::args_ok(1, 2, 1, norm::EVAL, false, false, 1e-5, 0.1));                         // evaluation without buffers
    CHECK(!norm::args_ok(1, 1, 1, 0, false, false, 1e-5, 0.1) && !norm::args_ok(1, 0, 1, norm::EVAL, false, true, 1e-5, 0.1));
    CHECK(!norm::args_ok(1, 2, 0, 0, false, false, 1e-5, 0.1) && !norm::args_ok(1, 2, 4097, 0, false, false, 1e-5, 0.1));
    CHECK(!norm::args_ok(0, 2, 1, 0, false, false, 1e-5, 0.1) && !norm::args_ok(1, 2, 1, 32, false, false, 1e-5, 0.1));
    for (double e : {0.0, -1e-5, nan, inf}) CHECK(!norm::args_ok(1, 2, 1, 0, false, false, e, 0.1));
    for (double m : {-0.1, 1.5, nan, inf}) CHECK(!norm::args_ok(1, 2, 1, 0, false, false, 1e-5, m));
}

// the mirror's loops on buffers of exactly the stated sizes
static void check_loops(int64_t L, int64_t N, int64_t F) {
    std::vector<float> x((size_t)(L * N * F)), gy(x.size()), y(x.size()), gx(x.size()), w((size_t)F), b((size_t)F), a((size_t)F), rm((size_t)F, 0.0f), rv((size_t)F, 1.0f);
    std::vector<float> gw((size_t)F), gb((size_t)F), gs((size_t)F);
    std::vector<double> stat((size_t)(L * 3 * F));
    uint64_t st = 0x9E3779B97F4A7C15ull * (uint64_t)(N + F);
    auto next = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((double)(st >> 11) / 9007199254740992.0 - 0.5); };
    for (auto& v : x) v = 4.0f * next() + 1.0f;
    for (auto& v : gy) v = next();
    for (int64_t k = 0; k < F; ++k) { w[k] = 1.0f + next(); b[k] = next(); a[k] = 0.25f + 0.1f * next(); }
    for (int pre = 0; pre < 2; ++pre)
        for (int post : {0, (int)norm::POST_RELU, (int)norm::POST_PRELU, (int)(norm::POST_PRELU | norm::SLOPE_PER_CHANNEL)})
            for (int ev = 0; ev < 2; ++ev) {
                if (ev && N < 1) continue;
                const int flags = (pre ? norm::PRE_RELU : 0) | post | (ev ? norm::EVAL : 0);
                CHECK(norm_forward(x.data(), L, N, F, w.data(), b.data(), a.data(), rm.data(), rv.data(), 0.1, 1e-5, flags, y.data(), stat.data()) == 0);
                CHECK(norm_backward(x.data(), gy.data(), L, N, F, w.data(), b.data(), a.data(), rm.data(), rv.data(), 1e-5, flags, stat.data(),
                                    gx.data(), gw.data(), gb.data(), gs.data()) == 0);
                for (float v : y) if (!std::isfinite(v)) { ++failures; std::printf("FAILED y not finite, flags %d\n", flags); break; }
                for (float v : gx) if (!std::isfinite(v)) { ++failures; std::printf("FAILED gx not finite, flags %d\n", flags); break; }
            }
    CHECK(norm_forward(x.data(), L, N, F, nullptr, nullptr, nullptr, nullptr, nullptr, 0.1, 1e-5, 0, y.data(), stat.data()) == 0);
    CHECK(norm_backward(x.data(), gy.data(), L, N, F, nullptr, nullptr, nullptr, nullptr, nullptr, 1e-5, 0, stat.data(), gx.data(), nullptr, nullptr, nullptr) == 0);
    for (int64_t k = 0; k < F; ++k) {   // without parameters and activations a column of y has mean 0 and its gradient sums to 0
        double s = 0.0, g = 0.0;
        for (int64_t i = 0; i < N; ++i) { s += y[(size_t)(i * F + k)]; g += gx[(size_t)(i * F + k)]; }
        CHECK(std::fabs(s) <= 1e-4 * (double)N && std::fabs(g) <= 1e-4 * (double)N);
    }
}

int main(int argc, char** argv) {
    const int64_t nmax = argc > 1 ? std::atoll(argv[1]) : 600;
    long long sizes = 0;
    check_refusals();
    const int64_t wide[] = {100, 128, 252, 256, 260, 516, 1024, 4095, 4096};
    for (int64_t L : {1, 3})
        for (int aligned = 0; aligned < 2; ++aligned) {
            for (int64_t N = 1; N <= nmax; N += (N < 4 || (N % 256 >= 254 || N % 256 <= 2) ? 1 : 61))
                for (int64_t F = 1; F <= 70; ++F) { check_map(L, N, F, aligned != 0); ++sizes; }
            for (int64_t F : wide)
                for (int64_t N : {(int64_t)1, (int64_t)2, (int64_t)256, (int64_t)257, nmax}) { check_map(L, N, F, aligned != 0); ++sizes; }
        }
    check_map(2 * norm::MAX_GRID * norm::GROUP_WAVES + 1, 2, 4, true);   // a pass that strides twice over its items
    ++sizes;
    check_loops(1, 2, 1);
    check_loops(2, 257, 5);
    check_loops(3, 513, 33);
    std::printf("%lld sizes, %d failures\n", sizes, failures);
    return failures ? 1 : 0;
}
