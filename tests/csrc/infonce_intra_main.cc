// The index arithmetic of the InfoNCE calls with intraview negatives (rlap_amd/csrc/rlap_infonce.h) as a stand-alone program, built
// with -fsanitize=address,undefined by tests/test_infonce_intra_cpu.py: for every N up to the bound given on the command line it
// walks the workgroup map of the main kernel -- row blocks x parts, four waves, 64 lanes, 16 registers -- over BOTH streams (the
// other view, then the owner's own view) through arrays of exactly the sizes the library carves, so that an index out of range is an
// error of the sanitizer and a cell visited twice or never one of the program.  It checks that every owner row meets its own column
// exactly once in the intraview stream, that the masked variant skips exactly that meeting, and that the part sums of the two
// streams land in disjoint cells of the forward call's array.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rlap_infonce.h"

using namespace rlap;

static int64_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

// the forward call: the ab pass into zpart [0, P) x Np, the intraview pass into [P, 2P) x Np; the pair's two intraview passes into
// zintra [2, P, Np]
static void check_forward(int64_t N, int intraview) {
    const int64_t T = infonce::num_tiles(N), Np = infonce::padded_rows(N), RB = infonce::row_blocks(N), P = infonce::num_parts(N);
    CHECK(infonce::intra_z_parts(N) == 2 * P, "parts of %lld", (long long)N);
    std::vector<int> zpart((size_t)(infonce::intra_z_parts(N) * Np), 0), zintra((size_t)(2 * P * Np), 0);
    std::vector<int> met((size_t)(Np * Np), 0), own((size_t)Np, 0), kept((size_t)Np, 0);
    for (int pass = 0; pass < 2; ++pass) {   // 0: the other view, 1: the own view
        int* out = zpart.data() + (size_t)(pass * P * Np);
        for (int64_t wg = 0; wg < RB * P; ++wg) {
            const int64_t blk = wg % RB, part = wg / RB;
            for (int wave = 0; wave < infonce::BLOCK_TILES; ++wave) {
                const int64_t ot = blk * infonce::BLOCK_TILES + wave;
                if (ot >= T) continue;
                for (int lane = 0; lane < 64; ++lane) {
                    const int c = lane & 31, h = lane >> 5;
                    const int64_t orow = ot * infonce::TILE + c;
                    const int64_t skip = pass == 1 && intraview == infonce::INTRA_MASKED ? orow : -1;
                    for (int64_t t = infonce::part_begin(N, part); t < infonce::part_begin(N, part + 1); ++t)
                        for (int r = 0; r < 16; ++r) {
                            const int64_t srow = t * infonce::TILE + infonce::reg_row(r, h);
                            if (pass == 1) {
                                ++met[(size_t)(orow * Np + srow)];
                                if (srow == orow) ++own[(size_t)orow];
                                const bool in = srow < N && srow != skip;
                                CHECK(in == (srow < N && infonce::intra_member(intraview, orow, srow)), "membership of (%lld, %lld)", (long long)orow, (long long)srow);
                                if (in && srow == orow) ++kept[(size_t)orow];
                            }
                        }
                    if (h == 0) {
                        ++out[(size_t)(part * Np + orow)];
                        if (pass == 1) { ++zintra[(size_t)(part * Np + orow)]; ++zintra[(size_t)((P + part) * Np + orow)]; }   // view a, view b
                    }
                }
            }
        }
    }
    for (size_t e = 0; e < zpart.size(); ++e) CHECK(zpart[e] == 1, "part sum cell %zu of %lld written %d times", e, (long long)N, zpart[e]);
    for (size_t e = 0; e < zintra.size(); ++e) CHECK(zintra[e] == 1, "intraview cell %zu of %lld written %d times", e, (long long)N, zintra[e]);
    for (size_t e = 0; e < met.size(); ++e) CHECK(met[e] == 1, "pair %zu of %lld met %d times", e, (long long)N, met[e]);
    for (int64_t i = 0; i < Np; ++i) {
        CHECK(own[(size_t)i] == 1, "row %lld of %lld met its own column %d times", (long long)i, (long long)N, own[(size_t)i]);
        const int want = i < N && intraview == infonce::INTRA_ALL ? 1 : 0;
        CHECK(kept[(size_t)i] == want, "row %lld of %lld kept its own column %d times", (long long)i, (long long)N, kept[(size_t)i]);
    }
}

// the backward call: one accumulator a (owner tile, part), both streams' tiles staged from images of Np rows, the reciprocals read at
// the stream row, the accumulator stored once into partial [P, Np]
static void check_backward(int64_t N, int intraview) {
    const int64_t T = infonce::num_tiles(N), Np = infonce::padded_rows(N), RB = infonce::row_blocks(N), P = infonce::num_parts(N);
    std::vector<int> image((size_t)Np, 0), rz((size_t)Np, 1), partial((size_t)(P * Np), 0);
    std::vector<int> steps((size_t)Np, 0), masked((size_t)Np, 0);
    for (int64_t wg = 0; wg < RB * P; ++wg) {
        const int64_t blk = wg % RB, part = wg / RB;
        for (int wave = 0; wave < infonce::BLOCK_TILES; ++wave) {
            const int64_t ot = blk * infonce::BLOCK_TILES + wave;
            if (ot >= T) continue;
            for (int c = 0; c < 32; ++c) {
                const int64_t orow = ot * infonce::TILE + c;
                for (int pass = 0; pass < 2; ++pass) {
                    const int64_t skip = pass == 1 && intraview == infonce::INTRA_MASKED ? orow : -1;
                    for (int64_t t = infonce::part_begin(N, part); t < infonce::part_begin(N, part + 1); ++t)
                        for (int r = 0; r < 16; ++r)
                            for (int h = 0; h < 2; ++h) {
                                const int64_t srow = t * infonce::TILE + infonce::reg_row(r, h);
                                image[(size_t)srow] += rz[(size_t)srow];          // (both read at the stream row: within Np)
                                ++steps[(size_t)orow];
                                if (srow == skip) ++masked[(size_t)orow];
                            }
                }
                ++partial[(size_t)(part * Np + orow)];
            }
        }
    }
    for (size_t e = 0; e < partial.size(); ++e) CHECK(partial[e] == 1, "accumulator cell %zu of %lld stored %d times", e, (long long)N, partial[e]);
    for (int64_t i = 0; i < Np; ++i) {
        CHECK(steps[(size_t)i] == 2 * Np, "row %lld of %lld took %d chain steps, not %lld", (long long)i, (long long)N, steps[(size_t)i], (long long)(2 * Np));
        CHECK(masked[(size_t)i] == (intraview == infonce::INTRA_MASKED ? 1 : 0), "row %lld of %lld masked %d steps", (long long)i, (long long)N, masked[(size_t)i]);
    }
}

int main(int argc, char** argv) {
    const int64_t bound = argc > 1 ? std::atoll(argv[1]) : 300;
    CHECK(!infonce::intra_ok(0) && infonce::intra_ok(1) && infonce::intra_ok(2) && !infonce::intra_ok(3) && !infonce::intra_ok(-1), "the variants");
    for (int64_t N = 1; N <= bound; ++N)
        for (int v : {(int)infonce::INTRA_MASKED, (int)infonce::INTRA_ALL}) {
            check_forward(N, v);
            check_backward(N, v);
        }
    const int64_t big[] = {2708, 4133, 34493, 169343, 1000000, ((int64_t)1 << 31) - 1};
    for (int64_t N : big) CHECK(infonce::intra_z_parts(N) == 2 * infonce::num_parts(N) && infonce::intra_z_parts(N) <= 2 * infonce::TARGET_GROUPS, "parts of %lld", (long long)N);
    std::printf("%lld sizes, %lld failures\n", (long long)bound, (long long)failures);
    return failures ? 1 : 0;
}
