// The index arithmetic of the fused CCA-SSG loss (rlap_amd/csrc/rlap_cca.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_cca_cpu.py: for every N up to the bound given on the command line and F in
// {1, 31, 32, 33, 100, 512} it walks the parts, the workgroup map of the Gram kernel (block -> view, part, group; wave -> super-tile
// pair -> tiles), the workgroup map of the backward product, the padded sizes and the finish through arrays of exactly the sizes the
// library carves, so that an index out of range is an error of the sanitizer and a cell visited twice or never one of the program.
// For every F from 1 to 512: the super-tile pairs, the tiles their waves store, and the instances the launchers choose.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rlap_cca.h"

using namespace rlap;

static int64_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

static void check_reg_rows() {
    int seen[32];
    std::memset(seen, 0, sizeof seen);
    for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) {
            const int row = cca::reg_row(r, h);
            CHECK(row >= 0 && row < 32, "reg_row(%d, %d) = %d", r, h, row);
            if (row >= 0 && row < 32) ++seen[row];
        }
    for (int i = 0; i < 32; ++i) CHECK(seen[i] == 1, "row %d is held %d times", i, seen[i]);
}

static void check_pairs(int64_t F) {
    const int nft = cca::feature_tiles(F), nst = cca::super_tiles(F), np = cca::super_pairs(F), Fp = cca::padded_features(F);
    CHECK(Fp % 32 == 0 && Fp >= F && Fp < F + 32 && nft * 32 == Fp, "padded features of %lld", (long long)F);
    CHECK(nst * 2 >= nft && (nst - 1) * 2 < nft, "super tiles of %lld", (long long)F);
    CHECK(cca::pair_groups(F) * cca::GROUP_PAIRS >= np && (cca::pair_groups(F) - 1) * cca::GROUP_PAIRS < np, "pair groups of %lld", (long long)F);
    std::vector<int> seen((size_t)(nst * nst), 0);
    for (int q = 0; q < np; ++q) {
        int I = -1, J = -1;
        cca::pair_of(q, nst, &I, &J);
        CHECK(0 <= I && I <= J && J < nst, "pair %d of %lld = (%d, %d)", q, (long long)F, I, J);
        if (0 <= I && I <= J && J < nst) ++seen[(size_t)(I * nst + J)];
    }
    for (int I = 0; I < nst; ++I)
        for (int J = 0; J < nst; ++J) CHECK(seen[(size_t)(I * nst + J)] == (I <= J ? 1 : 0), "super pair (%d, %d) of %lld", I, J, (long long)F);
    // the tiles the waves store, over all pairs: inside the image, in the upper triangle, each exactly once -- a clamped tile (odd
    // nft: the second tile of the last super tile) is computed and not stored; the operands of every tile, stored or not, are inside
    std::vector<int> tiles((size_t)(nft * nft), 0);
    for (int q = 0; q < np; ++q) {
        int I = 0, J = 0;
        cca::pair_of(q, nst, &I, &J);
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                const int tk = cca::tile_of(I, a, nft), tl = cca::tile_of(J, b, nft);
                CHECK(tk >= 0 && tk < nft && tl >= 0 && tl < nft, "operand tiles (%d, %d) of %lld", tk, tl, (long long)F);
                if (!cca::tile_stored(I, J, a, b, nft)) continue;
                CHECK(tk == 2 * I + a && tl == 2 * J + b, "a stored tile of %lld is a clamped one", (long long)F);
                CHECK(tk <= tl, "stored tile (%d, %d) of %lld is below the diagonal", tk, tl, (long long)F);
                if (tk >= 0 && tk < nft && tl >= 0 && tl < nft) ++tiles[(size_t)(tk * nft + tl)];
            }
    }
    for (int tk = 0; tk < nft; ++tk)
        for (int tl = 0; tl < nft; ++tl)
            CHECK(tiles[(size_t)(tk * nft + tl)] == (tk <= tl ? 1 : 0), "tile (%d, %d) of %lld stored %d times", tk, tl, (long long)F, tiles[(size_t)(tk * nft + tl)]);
    // the rules of the launchers: instances they have, the smallest that hold nft; what a thread or wave of the instance indexes
    // (j < NV float4s; wave + 4 j, j < NCT column tiles) covers the live ones and stays inside its array
    const int nv = cca::gram_instance(nft), nct = cca::zr_instance(nft);
    const bool nv_known = nv == 1 || nv == 2 || nv == 4 || nv == 8 || nv == 16;
    CHECK(nv_known && nv >= nft && (nv == 1 || nv / 2 < nft), "Gram instance %d of %lld (%d tiles)", nv, (long long)F, nft);
    CHECK(nct >= 1 && nct <= 4 && 4 * nct >= nft && 4 * (nct - 1) < nft, "zr instance %d of %lld (%d tiles)", nct, (long long)F, nft);
    if (nv_known && nv >= nft && nct >= 1 && nct <= 4) {
        std::vector<int> pre((size_t)nv, 0), pre_zr((size_t)(4 * nct), 0), col((size_t)nft, 0);
        for (int j = 0; j < nv; ++j)
            if (j < nft) ++pre[(size_t)j];
        for (int j = 0; j < 4 * nct; ++j)
            if (j < nft) ++pre_zr[(size_t)j];
        for (int wave = 0; wave < 4; ++wave)
            for (int j = 0; j < nct; ++j)
                if (wave + 4 * j < nft) ++col[(size_t)(wave + 4 * j)];
        for (int j = 0; j < nft; ++j)
            CHECK(pre[(size_t)j] == 1 && pre_zr[(size_t)j] == 1 && col[(size_t)j] == 1, "tile %d of %lld: staged %d and %d times, owned %d times", j,
                  (long long)F, pre[(size_t)j], pre_zr[(size_t)j], col[(size_t)j]);
    }
}

static void check_nf(int64_t N, int64_t F, bool elements) {
    const int64_t T = cca::num_tiles(N), Np = cca::padded_rows(N), P = cca::num_parts(N, F);
    const int nft = cca::feature_tiles(F), nst = cca::super_tiles(F), np = cca::super_pairs(F), groups = cca::pair_groups(F);
    const int64_t Fp = cca::padded_features(F);
    CHECK(T == (N + 31) / 32 && Np == 32 * T && Np >= N && Np < N + 32, "tiles of %lld", (long long)N);
    CHECK(P >= 1 && P <= T && P <= cca::MAX_PARTS, "parts of (%lld, %lld): %lld", (long long)N, (long long)F, (long long)P);
    CHECK(cca::part_begin(N, F, 0) == 0 && cca::part_begin(N, F, P) == Np, "ends of the parts of (%lld, %lld)", (long long)N, (long long)F);
    // every row of the padded image once, through the parts and the row pairs of a step; the reads of a step stay inside the image
    std::vector<int> row((size_t)Np, 0);
    std::vector<float> image((size_t)(Np * Fp), 0.0f);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t r0 = cca::part_begin(N, F, p), r1 = cca::part_begin(N, F, p + 1);
        CHECK(r0 < r1 && r0 % 32 == 0 && r1 % 32 == 0, "part %lld of (%lld, %lld): [%lld, %lld)", (long long)p, (long long)N, (long long)F, (long long)r0, (long long)r1);
        for (int64_t base = r0; base < r1; base += cca::TILE) {
            float sum = 0.0f;
            for (int64_t v = 0; v < cca::TILE * Fp; ++v) sum += image[(size_t)(base * Fp + v)];   // what the staging reads
            CHECK(sum == 0.0f, "the image");
            for (int s = 0; s < cca::TILE / 2; ++s)
                for (int h = 0; h < 2; ++h) ++row[(size_t)(base + 2 * s + h)];
        }
    }
    for (int64_t i = 0; i < Np; ++i) CHECK(row[(size_t)i] == 1, "row %lld of (%lld, %lld) summed %d times", (long long)i, (long long)N, (long long)F, row[(size_t)i]);
    // the Gram kernel's workgroup map: every upper-triangle tile of every (view, part) stored once, no other
    std::vector<int> tiles((size_t)(2 * P * nft * nft), 0);
    std::vector<int8_t> cells(elements ? (size_t)(2 * P * Fp * Fp) : 0, 0);
    for (int64_t block = 0; block < 2 * P * groups; ++block) {
        int64_t b = block;
        const int grp = (int)(b % groups); b /= groups;
        const int part = (int)(b % P);
        const int view = (int)(b / P);
        CHECK(view >= 0 && view < 2, "view of block %lld", (long long)block);
        for (int wave = 0; wave < cca::GROUP_PAIRS; ++wave) {
            const int q = grp * cca::GROUP_PAIRS + wave;
            if (q >= np) continue;
            int I, J;
            cca::pair_of(q, nst, &I, &J);
            for (int a = 0; a < 2; ++a)
                for (int bb = 0; bb < 2; ++bb) {
                    const int tk = cca::tile_of(I, a, nft), tl = cca::tile_of(J, bb, nft);
                    CHECK(tk >= 0 && tk < nft && tl >= 0 && tl < nft, "operand tiles (%d, %d) of %lld", tk, tl, (long long)F);
                    if (!cca::tile_stored(I, J, a, bb, nft)) continue;
                    CHECK(tk == 2 * I + a && tl == 2 * J + bb && tk <= tl, "a stored tile is a clamped one");
                    ++tiles[(size_t)((((int64_t)view * P + part) * nft + tk) * nft + tl)];
                    if (!elements) continue;
                    for (int h = 0; h < 2; ++h)
                        for (int r = 0; r < 16; ++r)
                            for (int c = 0; c < 32; ++c)
                                ++cells[(size_t)((((int64_t)view * P + part) * Fp + tk * 32 + cca::reg_row(r, h)) * Fp + tl * 32 + c)];
                }
        }
    }
    for (int64_t vp = 0; vp < 2 * P; ++vp)
        for (int tk = 0; tk < nft; ++tk)
            for (int tl = 0; tl < nft; ++tl)
                CHECK(tiles[(size_t)((vp * nft + tk) * nft + tl)] == (tk <= tl ? 1 : 0), "tile (%d, %d) of (%lld, %lld) stored %d times", tk, tl,
                      (long long)N, (long long)F, tiles[(size_t)((vp * nft + tk) * nft + tl)]);
    // the finish reads the upper triangle alone, inside the carved array, and only cells that were written
    if (elements)
        for (int v = 0; v < 2; ++v)
            for (int64_t k = 0; k < F; ++k)
                for (int64_t l = 0; l < F; ++l) {
                    const int64_t kk = k < l ? k : l, ll = k < l ? l : k;
                    for (int64_t p = 0; p < P; ++p)
                        CHECK(cells[(size_t)(((v * P + p) * Fp + kk) * Fp + ll)] == 1, "the finish reads cell (%lld, %lld) of (%lld, %lld)", (long long)kk,
                              (long long)ll, (long long)N, (long long)F);
                }
    // the backward product: (view, row tile) per workgroup, wave w owns column tiles w, w + 4, ...: every cell of P once
    const int nct = (nft + 3) / 4;
    std::vector<int> ptile((size_t)(2 * T * nft), 0);
    for (int64_t block = 0; block < 2 * T; ++block) {
        const int view = (int)(block / T);
        const int64_t tile = block - view * T;
        for (int wave = 0; wave < 4; ++wave)
            for (int j = 0; j < nct; ++j) {
                const int ct = wave + 4 * j;
                if (ct >= nft) continue;
                ++ptile[(size_t)((view * T + tile) * nft + ct)];
                const int64_t last = (tile * 32 + cca::reg_row(15, 1)) * Fp + ct * 32 + 31;
                CHECK(last < Np * Fp, "P offset %lld of (%lld, %lld)", (long long)last, (long long)N, (long long)F);
            }
    }
    for (size_t e = 0; e < ptile.size(); ++e) CHECK(ptile[e] == 1, "P tile %zu of (%lld, %lld) written %d times", e, (long long)N, (long long)F, ptile[e]);
}

// the chunk finishes: chunk sums in arrays of num_chunks, then their sum, against the rule in one piece
static void check_finish(int64_t n) {
    std::vector<double> x((size_t)n), csum((size_t)spmm::num_chunks(n));
    for (int64_t i = 0; i < n; ++i) x[(size_t)i] = 1.0 / (double)(3 * i + 1) - 0.25;
    const auto f = [&](int64_t e) { return x[(size_t)e]; };
    for (int64_t k = 0; k < spmm::num_chunks(n); ++k) csum[(size_t)k] = spmm::chunk_sum(n, k, f, f);
    double total = 0.0;
    for (int64_t k = 0; k < spmm::num_chunks(n); ++k) total = total + csum[(size_t)k];
    const double whole = cca::rule_sum(n, f, f);
    CHECK(std::memcmp(&total, &whole, 8) == 0, "chunk finish of %lld", (long long)n);
}

int main(int argc, char** argv) {
    const int64_t bound = argc > 1 ? std::atoll(argv[1]) : 300;
    const int64_t fs[] = {1, 31, 32, 33, 100, 512};
    check_reg_rows();
    for (int64_t F = 1; F <= cca::MAX_F; ++F) check_pairs(F);
    for (int64_t N = 2; N <= bound; ++N) {
        for (int64_t F : fs) check_nf(N, F, F <= 100 || N % 64 == 1 || N == bound);
        check_finish(N);
    }
    for (int64_t F : fs) check_finish(F * F);
    // large N: the arithmetic stays in range (no arrays)
    const int64_t big[] = {2708, 34493, 169343, ((int64_t)1 << 31) - 1};
    for (int64_t N : big)
        for (int64_t F : fs) {
            const int64_t P = cca::num_parts(N, F), Np = cca::padded_rows(N);
            CHECK(P >= 1 && P <= cca::MAX_PARTS && cca::part_begin(N, F, P) == Np && cca::part_begin(N, F, 0) == 0, "parts of %lld", (long long)N);
            for (int64_t p = 0; p < P; ++p)
                CHECK(cca::part_begin(N, F, p) < cca::part_begin(N, F, p + 1) && cca::part_begin(N, F, p) % 32 == 0, "part %lld of %lld", (long long)p, (long long)N);
        }
    CHECK(cca::gram_instance(0) == 0 && cca::gram_instance(17) == 0 && cca::zr_instance(0) == 0 && cca::zr_instance(17) == 0, "no instance outside 1 .. 16 tiles");
    CHECK(cca::lambd_ok(0.0) && cca::lambd_ok(1e-3) && cca::lambd_ok(1e300), "lambd inside");
    CHECK(!cca::lambd_ok(-1e-9) && !cca::lambd_ok((double)NAN) && !cca::lambd_ok((double)INFINITY), "lambd outside");
    std::printf("%lld sizes, %lld failures\n", (long long)bound, (long long)failures);
    return failures ? 1 : 0;
}
