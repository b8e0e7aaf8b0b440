// edgedrop_main.cc -- the edge-dropping mirror (edgedrop_mirror.cc) as a stand-alone program with its own main, for a build with
// -fsanitize=address,undefined (tests/test_edge_drop_cpu.py): a comb with every lane edge of the list rule, a ring, a directed list
// with duplicates and loops, rows around the tile edges of the compaction, no rows at all, then malformed inputs, which the call
// refuses.  Prints one line per call; exits 0 when every call answered as expected.
#include <cstdio>
#include <cstring>
#include <vector>

#include "edgedrop_mirror.cc"

namespace {

struct Rows { std::vector<int64_t> src, dst; int64_t N; };

Rows comb() {
    const int deg[] = {0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513};
    Rows r;
    r.N = 12 + 513;
    for (int j = 0; j < 12; ++j)
        for (int k = 0; k < deg[j]; ++k) {
            r.src.push_back(12 + k); r.dst.push_back(j);
            r.src.push_back(j); r.dst.push_back(12 + k);
        }
    return r;
}

Rows ring(int64_t n) {
    Rows r;
    r.N = n;
    for (int64_t a = 0; a < n; ++a) {
        r.src.push_back(a); r.dst.push_back((a + 1) % n);
        r.src.push_back((a + 1) % n); r.dst.push_back(a);
    }
    return r;
}

Rows directed() {
    Rows r;
    r.src = {0, 1, 1, 2, 3, 3, 3, 4, 5, 5, 6, 2, 0, 8, 8, 4};
    r.dst = {1, 2, 2, 0, 3, 4, 4, 5, 5, 6, 0, 3, 1, 0, 1, 4};
    r.N = 9;
    return r;
}

Rows random_rows(int64_t E, int64_t n) {
    Rows r;
    r.N = n;
    uint64_t z = 88172645463325252ull + (uint64_t)E;
    for (int64_t e = 0; e < E; ++e) {
        z = mix64(z); r.src.push_back((int64_t)(z % (uint64_t)n));
        z = mix64(z); r.dst.push_back((int64_t)(z % (uint64_t)n));
    }
    return r;
}

int failures = 0;

// one call; `want` is 0 for success or the status of the refusal
void call(const char* what, const Rows& r, int scheme, int source, std::vector<double> p, int want, bool weighted = false, int64_t max_iter = 50) {
    const int64_t E = (int64_t)r.src.size(), K = (int64_t)p.size();
    const size_t KE = (size_t)(K > 0 ? K : 1) * (size_t)(E > 0 ? E : 1);
    std::vector<double> rows(3 * KE), q(KE), u(KE), c(r.N > 0 ? r.N : 1), nw(r.N > 0 ? r.N : 1), w(E > 0 ? E : 1, 1.5);
    std::vector<int64_t> ptr(K + 2);
    std::vector<uint8_t> mask(KE);
    int32_t iters = -1, conv = -1;
    const int64_t got = edgedrop_run(r.src.data(), r.dst.data(), weighted ? w.data() : nullptr, E, r.N, scheme, source, p.data(), K, 0.7, 11, 0.85,
                                     10, 1e-6, max_iter, rows.data(), ptr.data(), mask.data(), q.data(), u.data(), c.data(), nw.data(), &iters,
                                     &conv);
    if (want) {
        if (got == -want) std::printf("%s scheme %d: refused as expected (%d)\n", what, scheme, want);
        else { std::printf("%s scheme %d: FAILED, expected a refusal %d, got %lld\n", what, scheme, want, (long long)got); ++failures; }
        return;
    }
    int64_t kept = 0;
    for (size_t i = 0; i < (size_t)K * (size_t)E; ++i) kept += mask[i];
    if (got < 0 || got != kept || ptr[K] != got || ptr[0] != 0) {
        std::printf("%s scheme %d: FAILED, %lld rows, %lld kept\n", what, scheme, (long long)got, (long long)kept);
        ++failures;
        return;
    }
    std::printf("%s scheme %d source %d: ok (%lld rows, %d steps)\n", what, scheme, source, (long long)got, (int)iters);
}

}  // namespace

int main() {
    const Rows graphs[] = {comb(), ring(64), directed()};
    const char* names[] = {"comb", "ring", "directed"};
    for (int g = 0; g < 3; ++g)
        for (int scheme = 0; scheme < SCHEMES; ++scheme)
            for (int source = 0; source < 2; ++source) call(names[g], graphs[g], scheme, source, {0.3, 0.45}, 0, source == 1);
    for (int64_t E : {0, 1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 3 * ROW_TILE + 5})
        for (int K = 1; K <= 3; ++K) call("tile edge", random_rows(E, 97), UNIFORM, 0, std::vector<double>(K, 0.5), 0);
    call("no rows", random_rows(0, 5), DEGREE, 0, {0.5}, 0);
    call("no rows, no nodes", random_rows(0, 0), EIGENVECTOR, 0, {0.5}, 0);
    call("one step", graphs[0], EIGENVECTOR, 0, {0.5}, 0, false, 1);
    // malformed inputs
    Rows bad = directed();
    bad.dst[3] = 9;
    call("an id past the last node", bad, DEGREE, 0, {0.5}, REFUSE_RANGE);
    bad.dst[3] = -1;
    call("a negative id", bad, PAGERANK, 0, {0.5}, REFUSE_RANGE);
    Rows none = directed();
    none.N = 0;
    call("rows without nodes", none, UNIFORM, 0, {0.5}, REFUSE_RANGE);
    call("33 views", directed(), UNIFORM, 0, std::vector<double>(33, 0.5), REFUSE_TOO_LARGE);
    call("no view", directed(), UNIFORM, 0, {}, REFUSE_BAD_ARG);
    call("p = 1.5", directed(), UNIFORM, 0, {0.2, 1.5}, REFUSE_BAD_ARG);
    call("p = nan", directed(), DEGREE, 0, {NAN}, REFUSE_BAD_ARG);
    call("an unknown scheme", directed(), 4, 0, {0.5}, REFUSE_BAD_ARG);
    call("an unknown aggregation", directed(), DEGREE, 2, {0.5}, REFUSE_BAD_ARG);
    call("no step", directed(), EIGENVECTOR, 0, {0.5}, REFUSE_BAD_ARG, false, 0);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
