// nodesample_main.cc -- the node-sampling mirror (nodesample_mirror.cc) as a stand-alone program with its own main, for a build
// with -fsanitize=address,undefined (tests/test_node_sample_cpu.py): a directed list with duplicates, loops, a sink, an id without
// rows and a hub of 513 outgoing rows, rows around the tile edges of the compaction, bitmaps around the word edges, no rows at
// all, then malformed inputs, which the call refuses.  Prints one line per call; exits 0 when every call answered as expected.
#include <cstdio>
#include <vector>

#include "nodesample_mirror.cc"

namespace {

struct Rows { std::vector<int64_t> src, dst; int64_t N; };

Rows directed() {
    Rows r;
    r.src = {0, 1, 1, 2, 3, 3, 3, 4, 5, 5, 6, 2, 0, 8, 8, 4};
    r.dst = {1, 2, 2, 0, 3, 4, 4, 5, 5, 6, 9, 3, 1, 0, 1, 4};   // 9: a sink; 7: no rows
    r.N = 10 + 513;
    for (int j = 0; j < 513; ++j) { r.src.push_back(6); r.dst.push_back(10 + j); }   // the hub
    return r;
}

Rows random_rows(int64_t E, int64_t n) {
    Rows r;
    r.N = n;
    uint64_t z = 88172645463325252ull + (uint64_t)E;
    for (int64_t e = 0; e < E; ++e) {
        z = mix64(z); r.src.push_back(n ? (int64_t)(z % (uint64_t)n) : 0);
        z = mix64(z); r.dst.push_back(n ? (int64_t)(z % (uint64_t)n) : 0);
    }
    return r;
}

int failures = 0;

// one call; `want` is 0 for success or the status of the refusal
void call(const char* what, const Rows& r, int scheme, std::vector<double> p, std::vector<int64_t> seeds, int64_t L, int want, bool weighted = false) {
    const int64_t E = (int64_t)r.src.size(), K = (int64_t)(scheme == WALK ? seeds.size() : p.size());
    const size_t KE = (size_t)(K > 0 ? K : 1) * (size_t)(E > 0 ? E : 1), KN = (size_t)(K > 0 ? K : 1) * (size_t)(r.N > 0 ? r.N : 1);
    int64_t walkers = 0;
    for (int64_t s : seeds) walkers += s > 0 && s < (1 << 20) ? s : 0;
    std::vector<double> rows(3 * KE), w(E > 0 ? E : 1, 1.5);
    std::vector<int64_t> ptr(K + 2), walks((size_t)walkers * (size_t)(L > 0 && L <= 1024 ? L + 1 : 1) + 1);
    std::vector<uint8_t> mask(KN);
    const int64_t got = nodesample_run(r.src.data(), r.dst.data(), weighted ? w.data() : nullptr, E, r.N, scheme, p.data(), seeds.data(), K, L, 11,
                                       rows.data(), ptr.data(), mask.data(), scheme == WALK ? walks.data() : nullptr);
    if (want) {
        if (got == -want) std::printf("%s scheme %d: refused as expected (%d)\n", what, scheme, want);
        else { std::printf("%s scheme %d: FAILED, expected a refusal %d, got %lld\n", what, scheme, want, (long long)got); ++failures; }
        return;
    }
    int64_t kept = 0;
    for (int64_t k = 0; k < K; ++k)
        for (int64_t e = 0; e < E; ++e) kept += mask[k * r.N + r.src[e]] && mask[k * r.N + r.dst[e]];
    if (got < 0 || got != kept || ptr[K] != got || ptr[0] != 0) {
        std::printf("%s scheme %d: FAILED, %lld rows, %lld kept\n", what, scheme, (long long)got, (long long)kept);
        ++failures;
        return;
    }
    std::printf("%s scheme %d: ok (%lld rows)\n", what, scheme, (long long)got);
}

}  // namespace

int main() {
    const Rows g = directed();
    call("directed", g, DROP, {0.3, 0.45}, {}, 0, 0, true);
    for (int64_t L : {0, 1, 10})
        for (int64_t s : {0, 1, 63, 64, 65, 257}) call("directed", g, WALK, {}, {s, 5}, L, 0, L == 1);
    for (int64_t E : {0, 1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 3 * ROW_TILE + 5})
        for (int K = 1; K <= 3; ++K) {
            call("tile edge", random_rows(E, 97), DROP, std::vector<double>(K, 0.3), {}, 0, 0);
            call("tile edge", random_rows(E, 97), WALK, {}, std::vector<int64_t>(K, 40), 3, 0);
        }
    for (int64_t n : {1, 63, 64, 65, 129, 4097}) {
        call("word edge", random_rows(300, n), DROP, {0.5}, {}, 0, 0);
        call("word edge", random_rows(300, n), WALK, {}, {n / 2 + 1}, 4, 0);
    }
    call("no rows, no nodes", random_rows(0, 0), DROP, {0.5}, {}, 0, 0);
    call("no rows, no nodes, no walkers", random_rows(0, 0), WALK, {}, {0, 0}, 10, 0);
    // malformed inputs
    Rows bad = directed();
    bad.dst[3] = bad.N;
    call("an id past the last node", bad, DROP, {0.5}, {}, 0, REFUSE_RANGE);
    bad.dst[3] = -1;
    call("a negative id", bad, WALK, {}, {5}, 3, REFUSE_RANGE);
    Rows none = directed();
    none.N = 0;
    call("rows without nodes", none, DROP, {0.5}, {}, 0, REFUSE_RANGE);
    call("walkers without nodes", random_rows(0, 0), WALK, {}, {1}, 3, REFUSE_BAD_ARG);
    call("33 views", g, DROP, std::vector<double>(33, 0.5), {}, 0, REFUSE_TOO_LARGE);
    call("no view", g, DROP, {}, {}, 0, REFUSE_BAD_ARG);
    call("p = 1.5", g, DROP, {0.2, 1.5}, {}, 0, REFUSE_BAD_ARG);
    call("p = nan", g, DROP, {NAN}, {}, 0, REFUSE_BAD_ARG);
    call("an unknown scheme", g, 2, {0.5}, {}, 0, REFUSE_BAD_ARG);
    call("a negative walker count", g, WALK, {}, {3, -1}, 3, REFUSE_BAD_ARG);
    call("2^31 walkers", g, WALK, {}, {(int64_t)1 << 31}, 3, REFUSE_TOO_LARGE);
    call("a negative walk length", g, WALK, {}, {3}, -1, REFUSE_BAD_ARG);
    call("a walk of 1025 steps", g, WALK, {}, {3}, 1025, REFUSE_BAD_ARG);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
