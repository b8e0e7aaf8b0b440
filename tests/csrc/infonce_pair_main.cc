// The index arithmetic of the symmetric InfoNCE pair (rlap_amd/csrc/rlap_infonce.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_infonce_pair_cpu.py: for every N up to the bound given on the command line it walks the
// groups, the parts and their spans, the workgroup map of the forward main kernel with its column array, wave sums and flushes, the
// column-sum order and the carved arrays of both calls through arrays of exactly the sizes the library carves, so that an index out of
// range is an error of the sanitizer and a cell visited twice or never one of the program.  Two sizes beyond 262,144 rows walk the
// spans of a part that has more than one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rlap_infonce.h"

using namespace rlap;

static int64_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

static void check_split(int64_t N) {
    const int64_t T = infonce::num_tiles(N), RB = infonce::row_blocks(N);
    const int64_t G = infonce::pair_groups(N), P = infonce::pair_parts(N), S = infonce::pair_span_tiles(N);
    CHECK(G >= 1 && G <= RB && G <= infonce::PAIR_GROUPS, "groups of %lld: %lld", (long long)N, (long long)G);
    CHECK(P >= 1 && P <= T && P <= infonce::PAIR_WORKGROUPS, "parts of %lld: %lld", (long long)N, (long long)P);
    CHECK(infonce::pair_group_begin(N, 0) == 0 && infonce::pair_group_begin(N, G) == RB, "ends of the groups of %lld", (long long)N);
    CHECK(infonce::pair_part_begin(N, 0) == 0 && infonce::pair_part_begin(N, P) == T, "ends of the parts of %lld", (long long)N);
    CHECK(S >= 1 && S <= infonce::PAIR_SPAN_TILES, "span of %lld: %lld", (long long)N, (long long)S);
    for (int64_t g = 0; g < G; ++g) CHECK(infonce::pair_group_begin(N, g) < infonce::pair_group_begin(N, g + 1), "group %lld of %lld is empty", (long long)g, (long long)N);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t len = infonce::pair_part_begin(N, p + 1) - infonce::pair_part_begin(N, p);
        CHECK(len >= 1, "part %lld of %lld is empty", (long long)p, (long long)N);
        CHECK(len <= S || S == infonce::PAIR_SPAN_TILES, "part %lld of %lld is longer than the span", (long long)p, (long long)N);
    }
}

// the forward main kernel's walk, with arrays of the carved and the LDS sizes
static void check_walk(int64_t N) {
    const int64_t T = infonce::num_tiles(N), Np = infonce::padded_rows(N);
    const int64_t G = infonce::pair_groups(N), P = infonce::pair_parts(N), S = infonce::pair_span_tiles(N);
    std::vector<int> zpart((size_t)(P * Np), 0), colpart((size_t)(G * Np), 0), diag((size_t)Np, 0);
    std::vector<int> pairs((size_t)(Np * Np), 0);                     // (owner row, stream row) cells: each met once
    std::vector<int> blocks((size_t)infonce::row_blocks(N), 0), tiles((size_t)T, 0);
    for (int64_t g = 0; g < G; ++g)
        for (int64_t b = infonce::pair_group_begin(N, g); b < infonce::pair_group_begin(N, g + 1); ++b) ++blocks[(size_t)b];
    for (int64_t p = 0; p < P; ++p)
        for (int64_t t = infonce::pair_part_begin(N, p); t < infonce::pair_part_begin(N, p + 1); ++t) ++tiles[(size_t)t];
    for (size_t b = 0; b < blocks.size(); ++b) CHECK(blocks[b] == 1, "row block %zu of %lld is in %d groups", b, (long long)N, blocks[b]);
    for (size_t t = 0; t < tiles.size(); ++t) CHECK(tiles[t] == 1, "tile %zu of %lld is in %d parts", t, (long long)N, tiles[t]);
    for (int64_t wg = 0; wg < G * P; ++wg) {
        const int64_t group = wg % G, part = wg / G;
        const int64_t bb = infonce::pair_group_begin(N, group), be = infonce::pair_group_begin(N, group + 1);
        const int64_t tb = infonce::pair_part_begin(N, part), te = infonce::pair_part_begin(N, part + 1);
        std::vector<int> col((size_t)(infonce::TILE * S), 0), wsum((size_t)(infonce::BLOCK_TILES * infonce::TILE), 0);
        for (int64_t sb = tb; sb < te; sb += infonce::PAIR_SPAN_TILES) {
            const int64_t se = sb + infonce::PAIR_SPAN_TILES < te ? sb + infonce::PAIR_SPAN_TILES : te;
            const int64_t span_cols = (se - sb) * infonce::TILE;
            for (int64_t v = 0; v < span_cols; ++v) col[(size_t)v] = 0;
            for (int64_t blk = bb; blk < be; ++blk) {
                for (int64_t t = sb; t < se; ++t) {
                    for (int wave = 0; wave < infonce::BLOCK_TILES; ++wave) {
                        const int64_t ot = blk * infonce::BLOCK_TILES + wave;
                        for (int lane = 0; lane < 64; ++lane) {
                            const int c = lane & 31, h = lane >> 5;
                            if (ot >= T) {
                                if (lane < infonce::TILE) wsum[(size_t)(wave * infonce::TILE + lane)] = 0;
                                continue;
                            }
                            const int64_t orow = ot * infonce::TILE + c;
                            for (int r = 0; r < 16; ++r) {
                                const int64_t srow = t * infonce::TILE + infonce::reg_row(r, h);
                                ++pairs[(size_t)(orow * Np + srow)];
                                if (srow == orow) ++diag[(size_t)orow];
                                if (c == 0) wsum[(size_t)(wave * infonce::TILE + infonce::reg_row(r, h))] = 1;
                            }
                        }
                    }
                    for (int x = 0; x < infonce::TILE; ++x) {
                        const int64_t j = (t - sb) * infonce::TILE + x;
                        int s = col[(size_t)j];
                        for (int w = 0; w < infonce::BLOCK_TILES; ++w) s += wsum[(size_t)(w * infonce::TILE + x)];
                        col[(size_t)j] = s;
                    }
                }
                for (int wave = 0; wave < infonce::BLOCK_TILES; ++wave) {
                    const int64_t ot = blk * infonce::BLOCK_TILES + wave;
                    if (ot >= T) continue;
                    for (int c = 0; c < 32; ++c) {
                        const int64_t slot = part * Np + ot * infonce::TILE + c;
                        if (sb > tb) CHECK(zpart[(size_t)slot] >= 1, "a later span of %lld reads a part sum nobody wrote", (long long)N);
                        if (sb == tb) ++zpart[(size_t)slot];
                    }
                }
            }
            // every column of the span has taken every live owner tile of the group once
            int64_t live = 0;
            for (int64_t blk = bb; blk < be; ++blk)
                for (int wave = 0; wave < infonce::BLOCK_TILES; ++wave) live += blk * infonce::BLOCK_TILES + wave < T ? 1 : 0;
            for (int64_t v = 0; v < span_cols; ++v) {
                CHECK(col[(size_t)v] == live, "column %lld of a span of %lld took %d tiles, not %lld", (long long)v, (long long)N, col[(size_t)v], (long long)live);
                ++colpart[(size_t)(group * Np + sb * infonce::TILE + v)];
            }
        }
    }
    for (size_t e = 0; e < zpart.size(); ++e) CHECK(zpart[e] == 1, "part sum cell %zu of %lld written %d times", e, (long long)N, zpart[e]);
    for (size_t e = 0; e < colpart.size(); ++e) CHECK(colpart[e] == 1, "group sum cell %zu of %lld written %d times", e, (long long)N, colpart[e]);
    for (int64_t i = 0; i < Np; ++i) CHECK(diag[(size_t)i] == 1, "diagonal of row %lld of %lld met %d times", (long long)i, (long long)N, diag[(size_t)i]);
    for (size_t e = 0; e < pairs.size(); ++e) CHECK(pairs[e] == 1, "pair %zu of %lld met %d times", e, (long long)N, pairs[e]);
    // the finish: two lists of N rows, two lists of chunk sums
    const int64_t nc = spmm::num_chunks(N);
    std::vector<double> rows((size_t)(2 * N)), csum((size_t)(2 * nc));
    for (int64_t i = 0; i < 2 * N; ++i) rows[(size_t)i] = 1.0 / (double)(3 * i + 1) - 0.25;
    for (int64_t q = 0; q < 2 * nc; ++q) {
        const int64_t l = q / nc, k = q - l * nc;
        csum[(size_t)q] = spmm::chunk_sum(N, k, [](int64_t) { return 1.0; }, [&](int64_t e) { return rows[(size_t)(l * N + e)]; });
    }
    for (int64_t l = 0; l < 2; ++l) {
        double total = 0.0;
        for (int64_t k = 0; k < nc; ++k) total = total + csum[(size_t)(l * nc + k)];
        const double whole = spmm::list_sum(N, [](int64_t) { return 1.0; }, [&](int64_t e) { return rows[(size_t)(l * N + e)]; }, false, 0.0, 0.0);
        CHECK(std::memcmp(&total, &whole, 8) == 0, "chunk finish of list %lld of %lld", (long long)l, (long long)N);
    }
}

// the same walk without the (owner row, stream row) cells, for an N whose parts have more than one span: the column array stays
// within its LDS size, every group-sum cell is flushed once, and a part sum is written in the first span and read-modified after
static void check_spans(int64_t N) {
    const int64_t T = infonce::num_tiles(N), Np = infonce::padded_rows(N);
    const int64_t G = infonce::pair_groups(N), P = infonce::pair_parts(N), S = infonce::pair_span_tiles(N);
    std::vector<int> zpart((size_t)(P * Np), 0), colpart((size_t)(G * Np), 0);
    int64_t spans_max = 0;
    for (int64_t wg = 0; wg < G * P; ++wg) {
        const int64_t group = wg % G, part = wg / G;
        const int64_t bb = infonce::pair_group_begin(N, group), be = infonce::pair_group_begin(N, group + 1);
        const int64_t tb = infonce::pair_part_begin(N, part), te = infonce::pair_part_begin(N, part + 1);
        std::vector<int> col((size_t)(infonce::TILE * S), 0);
        int64_t spans = 0;
        for (int64_t sb = tb; sb < te; sb += infonce::PAIR_SPAN_TILES, ++spans) {
            const int64_t se = sb + infonce::PAIR_SPAN_TILES < te ? sb + infonce::PAIR_SPAN_TILES : te;
            const int64_t span_cols = (se - sb) * infonce::TILE;
            for (int64_t v = 0; v < span_cols; ++v) col[(size_t)v] = 1;
            for (int64_t blk = bb; blk < be; ++blk)
                for (int wave = 0; wave < infonce::BLOCK_TILES; ++wave) {
                    const int64_t ot = blk * infonce::BLOCK_TILES + wave;
                    if (ot >= T) continue;
                    for (int c = 0; c < 32; ++c) {
                        const int64_t slot = part * Np + ot * infonce::TILE + c;
                        CHECK(zpart[(size_t)slot] == spans, "part sum cell %lld of %lld before span %lld", (long long)slot, (long long)N, (long long)spans);
                        ++zpart[(size_t)slot];
                    }
                }
            for (int64_t v = 0; v < span_cols; ++v) colpart[(size_t)(group * Np + sb * infonce::TILE + v)] += col[(size_t)v];
        }
        spans_max = spans > spans_max ? spans : spans_max;
    }
    CHECK(spans_max >= 2, "%lld rows have no part of two spans", (long long)N);
    for (size_t e = 0; e < colpart.size(); ++e) CHECK(colpart[e] == 1, "group sum cell %zu of %lld written %d times", e, (long long)N, colpart[e]);
    for (size_t e = 0; e < zpart.size(); ++e) CHECK(zpart[e] >= 1 && zpart[e] <= spans_max, "part sum cell %zu of %lld written %d times", e, (long long)N, zpart[e]);
}

// the column-sum order on exact data: integers summed by tree32 and by the waves in order give the plain count
static void check_tree() {
    double v[32];
    for (int c = 0; c < 32; ++c) v[c] = (double)(c + 1);
    CHECK(infonce::tree32(v) == 528.0, "tree32 of 1 .. 32");
    for (int c = 0; c < 32; ++c) v[c] = c == 7 ? 3.0 : 0.0;
    CHECK(infonce::tree32(v) == 3.0, "tree32 of one value");
}

int main(int argc, char** argv) {
    const int64_t bound = argc > 1 ? std::atoll(argv[1]) : 300;
    check_tree();
    for (int64_t N = 1; N <= bound; ++N) {
        check_split(N);
        check_walk(N);
    }
    // large N: the arithmetic stays in range and the partial arrays within (512 + 16) Np doubles (no arrays)
    const int64_t big[] = {2708, 4133, 34493, 169343, 262144, 262145, 1000000, ((int64_t)1 << 31) - 1};
    for (int64_t N : big) {
        check_split(N);
        const int64_t Np = infonce::padded_rows(N);
        CHECK((infonce::pair_parts(N) + infonce::pair_groups(N)) * Np <= (infonce::PAIR_WORKGROUPS + infonce::PAIR_GROUPS) * Np, "partial arrays of %lld", (long long)N);
    }
    check_spans(262145);   // the first N with a part of two spans
    check_spans(300000);
    CHECK(infonce::pair_span_tiles(262144) == 256 && infonce::pair_span_tiles(169343) == 166, "the span of a part");
    std::printf("%lld sizes, %lld failures\n", (long long)bound, (long long)failures);
    return failures ? 1 : 0;
}
