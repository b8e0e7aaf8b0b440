// The host-side arithmetic of the readout (rlap_amd/csrc/rlap_readout.h: clamped ranges, chunk counts, bounds, the map from work item
// to (graph, chunk), the definition of an element, the dispatch rule of the launchers for every F up to 65,536) in a stand-alone program, built with g++ -fsanitize=address,undefined by
// tests/test_readout_cpu.py.  Reads tables from standard input, one a line: "<well formed 0/1> <N> <G> <G+1 entries>", and checks
// each exhaustively; prints "dispatch <cases> <narrow> <16 bytes a lane>", "table <chunks> <chunked graphs> <part chunks>" per table
// and "<n> failures" at the end.
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <vector>

#include "rlap_readout.h"

using namespace rlap;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void check_table(bool well_formed, int64_t N, const std::vector<int64_t>& np) {
    const int64_t G = (int64_t)np.size() - 1;
    std::vector<int64_t> choff((size_t)G + 1), poff((size_t)G + 1), s((size_t)G), n((size_t)G);
    int64_t total = 0, part = 0, chunked = 0, covered = 0;
    for (int64_t g = 0; g < G; ++g) {
        readout::graph_range(np.data(), g, N, &s[g], &n[g]);
        CHECK(s[g] >= 0 && n[g] >= 0 && s[g] + n[g] <= N);                   // whatever the table holds
        if (well_formed) CHECK(s[g] == np[g] && n[g] == np[g + 1] - np[g]);
        choff[g] = total;
        poff[g] = part;
        total += readout::graph_chunks(n[g]);
        part += readout::graph_part_chunks(n[g]);
        chunked += n[g] > spmm::CHUNK;
        CHECK(readout::graph_chunks(n[g]) == (n[g] + spmm::CHUNK - 1) / spmm::CHUNK);
        CHECK(readout::graph_part_chunks(n[g]) == (n[g] > spmm::CHUNK ? readout::graph_chunks(n[g]) : 0));
    }
    choff[G] = total;
    poff[G] = part;
    if (well_formed) {   // the bounds the grid and the arena are sized from
        CHECK(total <= readout::chunk_bound(N, G));
        CHECK(chunked <= readout::chunked_bound(N, G));
        CHECK(part <= readout::part_bound(N, G));
    }
    // every work item, in order: graph after graph, chunk after chunk; the rows of the chunks tile the graph
    int64_t g = 0, k = 0, og = -1, ok_ = -1;
    CHECK(!readout::item_of(choff.data(), G, -1, &og, &ok_));
    CHECK(!readout::item_of(choff.data(), G, total, &og, &ok_));
    CHECK(!readout::item_of(choff.data(), G, total + 7, &og, &ok_));
    for (int64_t q = 0; q < total; ++q) {
        while (k >= readout::graph_chunks(n[g])) { ++g; k = 0; }
        CHECK(readout::item_of(choff.data(), G, q, &og, &ok_));
        CHECK(og == g && ok_ == k);
        const int64_t b = spmm::chunk_begin(ok_), e = spmm::chunk_end(n[og], ok_);
        CHECK(b < e && e - b <= spmm::CHUNK && e <= n[og]);
        CHECK(b == (k == 0 ? 0 : spmm::chunk_end(n[og], k - 1)));
        if (k + 1 == readout::graph_chunks(n[og])) CHECK(e == n[og]);
        if (n[og] > spmm::CHUNK) CHECK(poff[og] + ok_ < part);
        covered += e - b;
        ++k;
    }
    int64_t nodes = 0;
    for (int64_t h = 0; h < G; ++h) nodes += n[h];
    CHECK(covered == nodes);
    if (well_formed) CHECK(nodes == N);
    std::printf("table %lld %lld %lld\n", (long long)total, (long long)chunked, (long long)part);
}

// the definition against the chunk rule written out, bit for bit
static void check_rule() {
    const int64_t sizes[] = {0, 1, 2, 255, 256, 257, 511, 512, 513, 1000};
    for (int64_t n : sizes) {
        std::vector<double> x((size_t)n);
        uint64_t st = 0x9E3779B97F4A7C15ull * (uint64_t)(n + 1);
        for (int64_t i = 0; i < n; ++i) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            x[i] = ((st >> 11) & 1 ? -1.0 : 1.0) * std::ldexp((double)(st >> 40), (int)((st >> 12) % 60) - 30);
        }
        double total = 0.0;
        for (int64_t b = 0; b < n; b += spmm::CHUNK) {
            double c = 0.0;
            for (int64_t i = b; i < b + spmm::CHUNK && i < n; ++i) c = c + 1.0 * x[i];
            total = total + c;
        }
        const double got = readout::graph_sum(n, [&](int64_t e) { return x[(size_t)e]; });
        CHECK(std::memcmp(&got, &total, 8) == 0);
        const double mean = readout::finish(got, n, true), want = n > 0 ? total / (double)n : 0.0;
        CHECK(std::memcmp(&mean, &want, 8) == 0);
        const double same = readout::finish(got, n, false);
        CHECK(std::memcmp(&same, &got, 8) == 0);
    }
}

// the dispatch rule of both launchers, for every F the exports accept, both element sizes and both alignments
static void check_dispatch() {
    long long cases = 0, narrow = 0, vec = 0;
    for (int elem = 4; elem <= 8; elem += 4) {
        const int64_t V = 16 / elem;
        for (int aligned = 0; aligned < 2; ++aligned) {
            for (int64_t F = 1; F <= 65536; ++F) {
                const readout::Dispatch d = readout::dispatch(F, elem, aligned != 0);
                bool ok = d.lanes >= 1 && d.lanes <= 64 * d.ftiles && d.lanes > 64 * (d.ftiles - 1);
                ok = ok && d.lg >= 0 && d.lg <= 6;
                ok = ok && (d.lg == 6 || ((int64_t)1 << d.lg) >= d.lanes);                  // a group holds the row's lanes (6: a wave a row)
                ok = ok && (d.lg == 0 || ((int64_t)1 << (d.lg - 1)) < d.lanes);             // ... and is the smallest that does
                if (d.lg < 6) {   // the staged kernel: C = 64 >> lg chunks of upp = 8 x lanes units fit the 64 lanes x 8 turns of a piece
                    ok = ok && d.lanes <= 32 && d.ftiles == 1 && (int64_t)(64 >> d.lg) * 8 * d.lanes <= 512;
                } else {
                    ok = ok && d.lanes > 32;
                }
                ok = ok && (!d.vec || (F % V == 0 && aligned)) && (d.vec || !(F % V == 0 && aligned));
                ok = ok && d.lanes == (d.vec ? F / V : F);
                if (!ok) { ++failures; std::printf("FAILED dispatch F=%lld elem=%d aligned=%d\n", (long long)F, elem, aligned); }
                ++cases; narrow += d.lg < 6; vec += d.vec;
            }
        }
    }
    std::printf("dispatch %lld %lld %lld\n", cases, narrow, vec);
}

int main() {
    check_rule();
    check_dispatch();
    int wf;
    int64_t N, G;
    int tables = 0;
    while (std::cin >> wf >> N >> G) {
        std::vector<int64_t> np((size_t)G + 1);
        for (auto& v : np) std::cin >> v;
        check_table(wf != 0, N, np);
        ++tables;
    }
    std::printf("%d tables, %d failures\n", tables, failures);
    return failures ? 1 : 0;
}
