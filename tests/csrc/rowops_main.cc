// The host-side arithmetic of the fused bias, activation and dropout pass (rlap_amd/csrc/rlap_rowops.h: the refusals, the coin's
// threshold, the map from work item, row range and lane to (layer, row, columns), the arena's size) and the mirror's loops
// (tests/csrc/rowops_mirror.cc) in a stand-alone program, built with g++ -fsanitize=address,undefined by tests/test_rowops_cpu.py.
// usage: rowops_main <largest N>.  Every (L, N, F, alignment) with L in {1, 3}, N up to the argument and F up to 70 (and a few wide
// ones) is checked exhaustively: with the split of the forward pass every (layer, row, column) belongs to exactly one lane of one
// row range of one item; with the split of a pass that leaves chunk sums every (layer, chunk, column) belongs to exactly one lane,
// with all the chunk's rows.  Prints "<n> sizes, <f> failures".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rowops_mirror.cc"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void check_map(int64_t L, int64_t N, int64_t F, bool aligned) {
    const readout::Dispatch d = norm::dispatch(F, aligned);
    const int64_t V = d.vec ? 4 : 1, nch = spmm::num_chunks(N), items = norm::num_items(L, N, d);
    CHECK(d.vec == (aligned && F % 4 == 0));
    CHECK(rowops::split_of(items, true) == 0 && rowops::split_of(items, false) == norm::apply_split(items));
    for (int sums = 0; sums < 2; ++sums) {
        const int sp = rowops::split_of(items, sums != 0);
        std::vector<int> seen((size_t)(L * N * F), 0), chunk_seen((size_t)(L * nch * F), 0);
        norm::Item it{};
        for (int64_t w = 0; w < (items << sp); ++w)
            for (int lane = 0; lane < 64; ++lane) {
                if (!norm::item_of(w >> sp, lane, L, N, F, d, &it)) continue;
                int64_t r0, r1;
                norm::split_rows(it, sp, w & ((1 << sp) - 1), &r0, &r1);
                if (r0 >= r1) continue;
                const bool ok = it.l >= 0 && it.l < L && it.f0 >= 0 && it.f0 + V <= F && r0 >= it.r0 && r1 <= it.r1 && r1 <= N && (!d.vec || it.f0 % 4 == 0);
                if (!ok) { ++failures; std::printf("FAILED item L=%lld N=%lld F=%lld w=%lld lane=%d\n", (long long)L, (long long)N, (long long)F, (long long)w, lane); continue; }
                if (sums) CHECK(r0 == it.r0 && r1 == it.r1);
                for (int64_t v = 0; v < V; ++v) {
                    ++chunk_seen[(size_t)((it.l * nch + it.q) * F + it.f0 + v)];
                    for (int64_t r = r0; r < r1; ++r) ++seen[(size_t)((it.l * N + r) * F + it.f0 + v)];
                }
            }
        for (int s : seen) if (s != 1) { ++failures; std::printf("FAILED cover L=%lld N=%lld F=%lld aligned=%d sums=%d\n", (long long)L, (long long)N, (long long)F, (int)aligned, sums); break; }
        if (sums)
            for (int s : chunk_seen) if (s != 1) { ++failures; std::printf("FAILED chunk cover L=%lld N=%lld F=%lld\n", (long long)L, (long long)N, (long long)F); break; }
    }
    CHECK(rowops::backward_bytes(L, N, F, 0) == 0);
    for (int planes = 1; planes <= 2; ++planes) {
        const int64_t bb = rowops::backward_bytes(L, N, F, planes);
        CHECK(bb % 256 == 0 && bb >= (planes * L * nch * F + planes * L * F) * 8 && bb < (planes * L * nch * F + planes * L * F) * 8 + 512);
    }
}

static void check_refusals() {
    const double nan = std::nan(""), inf = INFINITY;
    CHECK(rowops::args_ok(1, 1, 1, 0, false, 0.0) && rowops::args_ok(3, 2, 4096, rowops::ACT_RELU | rowops::TRAINING, false, 0.5));
    CHECK(rowops::args_ok(1, 2, 8, rowops::ACT_PRELU | rowops::SLOPE_PER_CHANNEL, true, 0.999999));
    CHECK(!rowops::args_ok(1, 2, 1, rowops::ACT_RELU | rowops::ACT_PRELU, true, 0.1));   // both activations
    CHECK(!rowops::args_ok(1, 2, 1, rowops::ACT_PRELU, false, 0.1));                     // PReLU without a slope
    CHECK(!rowops::args_ok(1, 2, 1, rowops::SLOPE_PER_CHANNEL, true, 0.1));              // per channel without PReLU
    CHECK(!rowops::args_ok(1, 0, 1, 0, false, 0.1) && !rowops::args_ok(0, 2, 1, 0, false, 0.1) && !rowops::args_ok(1, 2, 0, 0, false, 0.1));
    CHECK(!rowops::args_ok(1, 2, 4097, 0, false, 0.1) && !rowops::args_ok(1, 2, 1, 16, false, 0.1));
    for (double p : {-0.1, 1.0, 1.5, nan, inf, -inf}) CHECK(!rowops::args_ok(1, 2, 1, rowops::TRAINING, false, p));
    CHECK(rowops::threshold(0.5, 0) == 0 && rowops::threshold(0.5, rowops::TRAINING) == 32768 && rowops::threshold(0.0, rowops::TRAINING) == 0);
    CHECK(rowops::threshold(0.2, rowops::TRAINING) == 13107 && rowops::threshold(0.9999999, rowops::TRAINING) == 65535);
    CHECK(rowops::scale(0) == 1.0 && rowops::scale(32768) == 2.0 && std::isfinite(rowops::scale(65535)));
}

// the mirror's loops on buffers of exactly the stated sizes
static void check_loops(int64_t L, int64_t N, int64_t F) {
    std::vector<float> x((size_t)(L * N * F)), gy(x.size()), y(x.size()), y0(x.size()), gx(x.size()), b((size_t)F), a((size_t)F), gb((size_t)F), gs((size_t)F), g1(1);
    std::vector<uint8_t> keep(x.size());
    uint64_t st = 0x9E3779B97F4A7C15ull * (uint64_t)(N + F);
    auto next = [&] { st = st * 6364136223846793005ull + 1442695040888963407ull; return (float)((double)(st >> 11) / 9007199254740992.0 - 0.5); };
    for (auto& v : x) v = 4.0f * next() + 0.5f;
    for (auto& v : gy) v = next();
    for (int64_t k = 0; k < F; ++k) { b[k] = next(); a[k] = 0.25f + 0.1f * next(); }
    for (int act : {0, (int)rowops::ACT_RELU, (int)rowops::ACT_PRELU, (int)(rowops::ACT_PRELU | rowops::SLOPE_PER_CHANNEL)})
        for (int tr = 0; tr < 2; ++tr) {
            const int flags = act | (tr ? rowops::TRAINING : 0);
            const bool per = (act & rowops::SLOPE_PER_CHANNEL) != 0;
            CHECK(rowops_forward(x.data(), L, N, F, b.data(), a.data(), 0.2, 7, flags, y.data()) == 0);
            CHECK(rowops_backward(x.data(), gy.data(), L, N, F, b.data(), a.data(), 0.2, 7, flags, gx.data(), gb.data(), per ? gs.data() : g1.data()) == 0);
            rowops_mask(L, N, F, 0.2, 7, flags, keep.data());
            for (size_t e = 0; e < x.size(); ++e) {
                if (!std::isfinite(y[e]) || !std::isfinite(gx[e])) { ++failures; std::printf("FAILED not finite, flags %d\n", flags); break; }
                if (!keep[e] && (y[e] != 0.0f || gx[e] != 0.0f)) { ++failures; std::printf("FAILED a dropped element is not zero, flags %d\n", flags); break; }
                if (!tr && !keep[e]) { ++failures; std::printf("FAILED a coin without training\n"); break; }
            }
        }
    CHECK(rowops_forward(x.data(), L, N, F, nullptr, nullptr, 0.0, 7, rowops::TRAINING, y.data()) == 0);
    CHECK(rowops_forward(x.data(), L, N, F, nullptr, nullptr, 0.3, 9, 0, y0.data()) == 0);
    for (size_t e = 0; e < x.size(); ++e) CHECK(y[e] == x[e] && y0[e] == x[e]);   // the identity: nothing added, nothing dropped
    CHECK(rowops_backward(x.data(), gy.data(), L, N, F, nullptr, nullptr, 0.0, 7, 0, gx.data(), nullptr, nullptr) == 0);
    for (size_t e = 0; e < x.size(); ++e) CHECK(gx[e] == gy[e]);
    CHECK(rowops_backward(x.data(), gy.data(), L, N, F, nullptr, nullptr, 0.0, 7, 0, nullptr, gb.data(), nullptr) == 0);
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
    check_loops(1, 1, 1);
    check_loops(2, 257, 5);
    check_loops(3, 513, 33);
    std::printf("%lld sizes, %d failures\n", sizes, failures);
    return failures ? 1 : 0;
}
