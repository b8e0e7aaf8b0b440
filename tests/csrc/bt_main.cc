// The index arithmetic of the fused Barlow Twins loss (rlap_amd/csrc/rlap_bt.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_bt_cpu.py: for every N up to the bound given on the command line and F in
// {1, 31, 32, 33, 64, 65, 100, 129, 512} it walks the parts, the workgroup map of the cross kernel (block -> part, block row, group of
// block columns; wave -> super-tile pair -> tiles), the finish's reads, the workgroup map of the backward product and the padded
// sizes through arrays of exactly the sizes the library carves, so that an index out of range is an error of the sanitizer and a
// cell visited twice or never one of the program.  For every F from 1 to 512: the staging map of a workgroup (which float4 of
// which slab a thread fetches, where it lands in LDS) and the operands its waves read, through arrays of the slabs' sizes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rlap_bt.h"

using namespace rlap;

static int64_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

constexpr int THREADS = 256, A_COLS = 64;   // rlap_bt.hip's BT_THREADS and BT_A_COLS

// the staging map and the operand reads of every workgroup of a part (they depend on F alone)
static void check_staging(int64_t F) {
    const int nft = bt::feature_tiles(F), nst = bt::super_tiles(F), Fp = bt::padded_features(F);
    const int rg = bt::row_groups(F), groups = bt::pair_groups(F), NW = bt::cross_instance(nft);
    CHECK(Fp % 32 == 0 && Fp >= F && Fp < F + 32 && nft * 32 == Fp, "padded features of %lld", (long long)F);
    CHECK(nst * 2 >= nft && (nst - 1) * 2 < nft, "super tiles of %lld", (long long)F);
    CHECK(rg * bt::GROUP_PAIRS >= nst && (rg - 1) * bt::GROUP_PAIRS < nst && groups == nst * rg, "groups of %lld", (long long)F);
    CHECK((NW == 1 || NW == 2 || NW == 4) && NW >= (nst < bt::GROUP_PAIRS ? nst : bt::GROUP_PAIRS), "cross instance %d of %lld", NW, (long long)F);
    if (!(NW == 1 || NW == 2 || NW == 4)) return;
    const int BW = 64 * NW, AV = A_COLS / 4, BV = BW / 4;
    std::vector<float> rows((size_t)(32 * Fp), 0.0f);                 // 32 rows of either image: what a step reads
    std::vector<int> pairs((size_t)(nst * nst), 0);
    for (int grp = 0; grp < groups; ++grp) {
        int I = -1, J0 = -1;
        bt::group_of(grp, rg, &I, &J0);
        CHECK(0 <= I && I < nst && 0 <= J0 && J0 < nst && J0 % bt::GROUP_PAIRS == 0, "group %d of %lld = (%d, %d)", grp, (long long)F, I, J0);
        std::vector<int8_t> sa((size_t)(32 * A_COLS), 0), sb((size_t)(32 * BW), 0);   // 0 never written, 1 from the image, 2 zeros
        for (int tid = 0; tid < THREADS; ++tid) {
            for (int j = 0; j < 2; ++j) {
                const int v = tid + THREADS * j, col = A_COLS * I + 4 * (v % AV), row = v / AV;
                CHECK(row >= 0 && row < 32, "row %d of the z1 slab", row);
                float sum = 0.0f;
                if (col < Fp)
                    for (int e = 0; e < 4; ++e) sum += rows[(size_t)(row * Fp + col + e)];
                CHECK(sum == 0.0f, "the image");
                for (int e = 0; e < 4; ++e) {
                    CHECK(sa[(size_t)(4 * v + e)] == 0, "float %d of the z1 slab staged twice", 4 * v + e);
                    sa[(size_t)(4 * v + e)] = col < Fp ? 1 : 2;
                }
                CHECK(4 * v == row * A_COLS + (col - A_COLS * I), "the z1 slab is row-major");
            }
            for (int j = 0; j < 2 * NW; ++j) {
                const int v = tid + THREADS * j, col = A_COLS * J0 + 4 * (v % BV), row = v / BV;
                CHECK(row >= 0 && row < 32, "row %d of the z2 slab", row);
                float sum = 0.0f;
                if (col < Fp)
                    for (int e = 0; e < 4; ++e) sum += rows[(size_t)(row * Fp + col + e)];
                CHECK(sum == 0.0f, "the image");
                for (int e = 0; e < 4; ++e) {
                    CHECK(sb[(size_t)(4 * v + e)] == 0, "float %d of the z2 slab staged twice", 4 * v + e);
                    sb[(size_t)(4 * v + e)] = col < Fp ? 1 : 2;
                }
                CHECK(4 * v == row * BW + (col - A_COLS * J0), "the z2 slab is row-major");
            }
        }
        for (size_t e = 0; e < sa.size(); ++e) CHECK(sa[e] != 0, "float %zu of the z1 slab never staged", e);
        for (size_t e = 0; e < sb.size(); ++e) CHECK(sb[e] != 0, "float %zu of the z2 slab never staged", e);
        for (int wave = 0; wave < bt::GROUP_PAIRS; ++wave) {
            if (!(wave < NW && bt::wave_active(J0, wave, nst))) continue;
            const int J = J0 + wave;
            ++pairs[(size_t)(I * nst + J)];
            for (int t = 0; t < 2; ++t) {
                const int ka = bt::tile_of(I, t, nft) * 32 - A_COLS * I, kb = bt::tile_of(J, t, nft) * 32 - A_COLS * J0;
                for (int s = 0; s < 16; ++s)
                    for (int h = 0; h < 2; ++h)
                        for (int c = 0; c < 32; ++c) {
                            CHECK(sa[(size_t)(h * A_COLS + c + 2 * s * A_COLS + ka)] == 1, "an A operand of (%d, %d) of %lld is not from the image", I, J, (long long)F);
                            CHECK(sb[(size_t)(h * BW + c + 2 * s * BW + kb)] == 1, "a B operand of (%d, %d) of %lld is not from the image", I, J, (long long)F);
                        }
            }
        }
    }
    for (int e = 0; e < nst * nst; ++e) CHECK(pairs[(size_t)e] == 1, "super pair %d of %lld owned %d times", e, (long long)F, pairs[(size_t)e]);
    // the backward instance: what a thread or wave of it indexes covers the live tiles and stays inside its array
    const int nct = bt::zr_instance(nft);
    CHECK(nct >= 1 && nct <= 4 && 4 * nct >= nft && 4 * (nct - 1) < nft, "zr instance %d of %lld (%d tiles)", nct, (long long)F, nft);
}

static void check_nf(int64_t N, int64_t F, bool elements) {
    const int64_t T = bt::num_tiles(N), Np = bt::padded_rows(N), P = bt::num_parts(N, F);
    const int nft = bt::feature_tiles(F), nst = bt::super_tiles(F), rg = bt::row_groups(F), groups = bt::pair_groups(F);
    const int NW = bt::cross_instance(nft);
    const int64_t Fp = bt::padded_features(F);
    CHECK(T == (N + 31) / 32 && Np == 32 * T && Np >= N && Np < N + 32, "tiles of %lld", (long long)N);
    CHECK(P >= 1 && P <= T && P <= bt::MAX_PARTS, "parts of (%lld, %lld): %lld", (long long)N, (long long)F, (long long)P);
    CHECK(bt::part_begin(N, F, 0) == 0 && bt::part_begin(N, F, P) == Np, "ends of the parts of (%lld, %lld)", (long long)N, (long long)F);
    // every row of the padded image once, through the parts and the row pairs of a step; the reads of a step stay inside the image
    std::vector<int> row((size_t)Np, 0);
    std::vector<float> image((size_t)(Np * Fp), 0.0f);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t r0 = bt::part_begin(N, F, p), r1 = bt::part_begin(N, F, p + 1);
        CHECK(r0 < r1 && r0 % 32 == 0 && r1 % 32 == 0, "part %lld of (%lld, %lld): [%lld, %lld)", (long long)p, (long long)N, (long long)F, (long long)r0, (long long)r1);
        for (int64_t base = r0; base < r1; base += bt::TILE) {
            float sum = 0.0f;
            for (int64_t v = 0; v < bt::TILE * Fp; ++v) sum += image[(size_t)(base * Fp + v)];   // what the staging of all groups reads
            CHECK(sum == 0.0f, "the image");
            for (int s = 0; s < bt::TILE / 2; ++s)
                for (int h = 0; h < 2; ++h) ++row[(size_t)(base + 2 * s + h)];
        }
    }
    for (int64_t i = 0; i < Np; ++i) CHECK(row[(size_t)i] == 1, "row %lld of (%lld, %lld) summed %d times", (long long)i, (long long)N, (long long)F, row[(size_t)i]);
    // the cross kernel's workgroup map: every tile of the full grid of every part stored once, no other
    std::vector<int> tiles((size_t)(P * nft * nft), 0);
    std::vector<int8_t> cells(elements ? (size_t)(P * Fp * Fp) : 0, 0);
    for (int64_t block = 0; block < P * groups; ++block) {
        const int grp = (int)(block % groups);
        const int part = (int)(block / groups);
        CHECK(part >= 0 && part < P, "part of block %lld", (long long)block);
        int I, J0;
        bt::group_of(grp, rg, &I, &J0);
        for (int wave = 0; wave < bt::GROUP_PAIRS; ++wave) {
            if (!(wave < NW && bt::wave_active(J0, wave, nst))) continue;
            const int J = J0 + wave;
            for (int a = 0; a < 2; ++a)
                for (int bb = 0; bb < 2; ++bb) {
                    const int tk = bt::tile_of(I, a, nft), tl = bt::tile_of(J, bb, nft);
                    CHECK(tk >= 0 && tk < nft && tl >= 0 && tl < nft, "operand tiles (%d, %d) of %lld", tk, tl, (long long)F);
                    if (!bt::tile_stored(I, J, a, bb, nft)) continue;
                    CHECK(tk == 2 * I + a && tl == 2 * J + bb, "a stored tile is a clamped one");
                    ++tiles[(size_t)((((int64_t)part * nft) + tk) * nft + tl)];
                    if (!elements) continue;
                    for (int h = 0; h < 2; ++h)
                        for (int r = 0; r < 16; ++r)
                            for (int c = 0; c < 32; ++c)
                                ++cells[(size_t)(((int64_t)part * Fp + (2 * I + a) * 32 + bt::reg_row(r, h)) * Fp + (2 * J + bb) * 32 + c)];
                }
        }
    }
    for (int64_t p = 0; p < P; ++p)
        for (int tk = 0; tk < nft; ++tk)
            for (int tl = 0; tl < nft; ++tl)
                CHECK(tiles[(size_t)((p * nft + tk) * nft + tl)] == 1, "tile (%d, %d) of (%lld, %lld) stored %d times", tk, tl, (long long)N, (long long)F,
                      tiles[(size_t)((p * nft + tk) * nft + tl)]);
    if (elements) {
        // the carved array element by element: every cell written exactly once
        for (size_t e = 0; e < cells.size(); ++e) CHECK(cells[e] == 1, "cell %zu of (%lld, %lld) written %d times", e, (long long)N, (long long)F, (int)cells[e]);
        // the finish reads every (k, l) of every part, inside the carved array
        for (int64_t k = 0; k < F; ++k)
            for (int64_t l = 0; l < F; ++l)
                for (int64_t p = 0; p < P; ++p)
                    CHECK(cells[(size_t)((p * Fp + k) * Fp + l)] == 1, "the finish reads cell (%lld, %lld) of (%lld, %lld)", (long long)k, (long long)l, (long long)N, (long long)F);
    }
    // the backward product: (product, row tile) per workgroup, wave w owns column tiles w, w + 4, ...: every cell of P once
    const int nct = bt::zr_instance(nft);
    std::vector<int> ptile((size_t)(2 * T * nft), 0);
    for (int64_t block = 0; block < 2 * T; ++block) {
        const int view = (int)(block / T);
        const int64_t tile = block - view * T;
        for (int wave = 0; wave < 4; ++wave)
            for (int j = 0; j < nct; ++j) {
                const int ct = wave + 4 * j;
                if (ct >= nft) continue;
                ++ptile[(size_t)((view * T + tile) * nft + ct)];
                const int64_t last = (tile * 32 + bt::reg_row(15, 1)) * Fp + ct * 32 + 31;
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
    const double whole = bt::rule_sum(n, f, f);
    CHECK(std::memcmp(&total, &whole, 8) == 0, "chunk finish of %lld", (long long)n);
}

int main(int argc, char** argv) {
    const int64_t bound = argc > 1 ? std::atoll(argv[1]) : 300;
    const int64_t fs[] = {1, 31, 32, 33, 64, 65, 100, 129, 512};
    for (int64_t F = 1; F <= bt::MAX_F; ++F) check_staging(F);
    for (int64_t N = 2; N <= bound; ++N) {
        for (int64_t F : fs) check_nf(N, F, F <= 129 || N % 64 == 1 || N == bound);
        check_finish(N);
    }
    for (int64_t F : fs) { check_finish(F * F); check_finish(F); }
    // the chunk sums of a call fit the arrays of the terms kernel
    CHECK(spmm::num_chunks((int64_t)bt::MAX_F * bt::MAX_F) == bt::MAX_F * bt::MAX_F / spmm::CHUNK && spmm::num_chunks(bt::MAX_F) == bt::MAX_F / spmm::CHUNK,
          "the chunks of the largest call");
    // large N: the arithmetic stays in range (no arrays)
    const int64_t big[] = {2708, 34493, 169343, ((int64_t)1 << 31) - 1};
    for (int64_t N : big)
        for (int64_t F : fs) {
            const int64_t P = bt::num_parts(N, F), Np = bt::padded_rows(N);
            CHECK(P >= 1 && P <= bt::MAX_PARTS && bt::part_begin(N, F, P) == Np && bt::part_begin(N, F, 0) == 0, "parts of %lld", (long long)N);
            for (int64_t p = 0; p < P; ++p)
                CHECK(bt::part_begin(N, F, p) < bt::part_begin(N, F, p + 1) && bt::part_begin(N, F, p) % 32 == 0, "part %lld of %lld", (long long)p, (long long)N);
        }
    CHECK(bt::cross_instance(0) == 0 && bt::cross_instance(17) == 0 && bt::zr_instance(0) == 0 && bt::zr_instance(17) == 0, "no instance outside 1 .. 16 tiles");
    CHECK(bt::lambd_ok(0.0) && bt::lambd_ok(1e-3) && bt::lambd_ok(1e300) && bt::eps_ok(0.0) && bt::eps_ok(1e-15), "lambd and eps inside");
    CHECK(!bt::lambd_ok(-1e-9) && !bt::lambd_ok((double)NAN) && !bt::lambd_ok((double)INFINITY) && !bt::eps_ok(-1e-30) && !bt::eps_ok((double)NAN) &&
              !bt::eps_ok((double)INFINITY), "lambd and eps outside");
    CHECK(bt::flags_ok(0) && bt::flags_ok(bt::NO_STANDARDIZE) && !bt::flags_ok(2) && !bt::flags_ok(1 << 20) && !bt::flags_ok(-1), "flags");
    std::printf("%lld sizes, %lld failures\n", (long long)bound, (long long)failures);
    return failures ? 1 : 0;
}
