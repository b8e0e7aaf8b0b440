// The tile and group table of the PPR diffusion (rlap_amd/csrc/rlap_ppr_tiles.h: the tile area, the table's capacity, where every tile
// lies and which tiles run together) in a stand-alone program, built with g++ -fsanitize=address,undefined by
// tests/test_ppr_tiles_cpu.py.  Reads lists of segment sizes from standard input, one a line: "<S> <S node counts>", and checks each
// with bcap equal to the sum of the sizes and with larger ones; prints "list <tiles> <groups> <small tiles> <large tiles> <largest
// group's rows>" per list and "<n> lists, <f> failures" at the end.
#include <stdint.h>

#include <cstdio>
#include <iostream>
#include <vector>

#include "rlap_ppr_tiles.h"

using namespace rlap;
using namespace rlap::pprtiles;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (++failures <= 50) std::printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void check_list(const std::vector<int64_t>& nodes, int64_t bcap, bool print) {
    const int64_t S = (int64_t)nodes.size();
    const Sizes z = sizes(bcap, S);
    Table t;
    build(nodes.data(), S, &t);
    const int64_t ntiles = t.ntiles(), ngroups = t.ngroups();
    CHECK(z.area == area_elems(bcap));
    CHECK((int64_t)t.tab.size() == ntiles * T_FIELDS);
    CHECK((int64_t)t.gsmall.size() == ngroups && (int64_t)t.grows.size() == ngroups);
    CHECK(ntiles <= z.tcap);
    CHECK(fits(t, z, nodes.data()));                              // what the run itself checks
    // every (segment, c0): exactly once
    std::vector<int64_t> first((size_t)S + 1, 0);
    for (int64_t s = 0; s < S; ++s) first[(size_t)s + 1] = first[(size_t)s] + (nodes[(size_t)s] + PPR_TILE - 1) / PPR_TILE;
    CHECK(ntiles == first[(size_t)S]);
    std::vector<char> seen((size_t)first[(size_t)S], 0);
    int64_t small = 0, large = 0, max_rows = 0;
    bool large_seen = false;
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t u0 = t.gstart[(size_t)g], u1 = g + 1 < ngroups ? t.gstart[(size_t)g + 1] : ntiles;
        CHECK(u0 < u1 && u1 <= ntiles);                           // no empty group
        CHECK(g == 0 ? u0 == 0 : u0 > t.gstart[(size_t)g - 1]);
        CHECK(u1 - u0 <= GROUP_TILES);
        int64_t rows = 0, end = 0, bytes = 0;                     // end: first free element after the tiles so far
        for (int64_t u = u0; u < u1 && u < ntiles; ++u) {
            const int64_t* d = t.tab.data() + u * T_FIELDS;
            const int64_t s = d[T_SEG], c0 = d[T_C0];
            CHECK(s >= 0 && s < S);
            if (s < 0 || s >= S) continue;
            const int64_t n = nodes[(size_t)s];
            CHECK(n > 0 && c0 >= 0 && c0 < n && c0 % PPR_TILE == 0);
            const int64_t slot = first[(size_t)s] + c0 / PPR_TILE;
            if (c0 >= 0 && c0 < n && c0 % PPR_TILE == 0) { CHECK(!seen[(size_t)slot]); seen[(size_t)slot] = 1; }
            CHECK(d[T_XOFF] >= end);                              // tiles of one group do not overlap (and ascend)
            CHECK(d[T_XOFF] >= 0 && d[T_XOFF] + 2 * PPR_TILE * n <= z.area);
            end = d[T_XOFF] + 2 * PPR_TILE * n;
            CHECK(d[T_ROFF] == rows);                             // from 0 in steps of n_s
            rows += n;
            bytes += 2 * PPR_TILE * n * (int64_t)sizeof(double);
            const bool is_small = n <= PPR_SMALL_MAX;
            CHECK((t.gsmall[(size_t)g] != 0) == is_small);
            if (is_small) { CHECK(!large_seen); ++small; } else { large_seen = true; ++large; }
        }
        CHECK(t.grows[(size_t)g] == rows);
        CHECK(rows <= z.area_rows);
        if (u1 - u0 > 1) CHECK(bytes <= (int64_t)PPR_TILE_BUDGET);
        if (rows > max_rows) max_rows = rows;
    }
    for (char c : seen) CHECK(c == 1);
    CHECK(small == t.small_tiles && large == t.large_tiles && small + large == ntiles);
    if (print)
        std::printf("list %lld %lld %lld %lld %lld\n", (long long)ntiles, (long long)ngroups, (long long)small, (long long)large, (long long)max_rows);
}

// the tile area: at least one tile of all the blocks, at most max(that, the budget), and no overflow up to the largest row count
static void check_area() {
    const int64_t budget = (int64_t)(PPR_TILE_BUDGET / sizeof(double));
    const int64_t caps[] = {0, 1, 63, 64, 65, 1023, 1024, 1025, 4096, 1048576, 1048577, 1100000, ((int64_t)1 << 31) - 2, (int64_t)1 << 40};
    for (int64_t b : caps) {
        const int64_t one = 2 * PPR_TILE * b, a = area_elems(b);
        CHECK(a >= one && a <= (one > budget ? one : budget));
        const int64_t tiles = (b + PPR_TILE - 1) / PPR_TILE;
        if (b <= 1100000) CHECK(a == (one * tiles < budget ? (one > one * tiles ? one : one * tiles) : (one > budget ? one : budget)));
        else CHECK(a == one);
    }
}

int main() {
    check_area();
    int64_t S;
    int lists = 0;
    while (std::cin >> S) {
        std::vector<int64_t> nodes((size_t)S);
        int64_t sum = 0;
        for (auto& v : nodes) { std::cin >> v; sum += v; }
        check_list(nodes, sum, true);
        check_list(nodes, sum + 1, false);
        check_list(nodes, 2 * sum + 1000, false);
        check_list(nodes, 64 * sum + 12345, false);
        ++lists;
    }
    std::printf("%d lists, %d failures\n", lists, failures);
    return failures ? 1 : 0;
}
