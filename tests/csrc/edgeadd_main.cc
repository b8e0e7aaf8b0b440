// edgeadd_main.cc -- the edge-adding mirror (edgeadd_mirror.cc) as a stand-alone program with its own main, for a build with
// -fsanitize=address,undefined (tests/test_edge_add_cpu.py): random rows with duplicates and loops around the tile edges of the
// merge, coalesced and not, 1 to 3 views, the widest keys, no rows at all, then malformed inputs, which the call refuses.  Prints
// one line per call; exits 0 when every call answered as expected.
#include <cstdio>
#include <vector>

#include "edgeadd_mirror.cc"

namespace {

struct Rows { std::vector<int64_t> src, dst; int64_t N; };

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
void call(const char* what, const Rows& r, std::vector<int64_t> num_add, int coalesce, int want, bool weighted = false, bool with_added = true) {
    const int64_t E = (int64_t)r.src.size(), K = (int64_t)num_add.size();
    int64_t all_added = 0;
    for (int64_t c : num_add) all_added += c > 0 && c < (1 << 24) ? c : 0;
    std::vector<double> rows(3 * ((size_t)(K > 0 ? K : 1) * (size_t)E + (size_t)all_added) + 3), w(E > 0 ? E : 1, 1.5);
    std::vector<int64_t> ptr(K + 2), added(2 * (size_t)all_added + 2), aptr(K + 2), stats(2);
    const int64_t got = edgeadd_run(r.src.data(), r.dst.data(), weighted ? w.data() : nullptr, E, r.N, num_add.data(), K, 11, coalesce, rows.data(),
                                    ptr.data(), with_added ? added.data() : nullptr, with_added ? aptr.data() : nullptr, stats.data());
    if (want) {
        if (got == -want) std::printf("%s: refused as expected (%d)\n", what, want);
        else { std::printf("%s: FAILED, expected a refusal %d, got %lld\n", what, want, (long long)got); ++failures; }
        return;
    }
    bool ok = got >= 0 && ptr[0] == 0 && ptr[K] == got && got <= K * E + all_added && (coalesce || got == K * E + all_added);
    for (int64_t k = 0; ok && coalesce && k < K; ++k)
        for (int64_t p = ptr[k] + 1; ok && p < ptr[k + 1]; ++p)
            ok = rows[3 * (p - 1)] < rows[3 * p] || (rows[3 * (p - 1)] == rows[3 * p] && rows[3 * (p - 1) + 1] < rows[3 * p + 1]);
    double mass = 0.0;
    for (int64_t p = 0; p < got; ++p) mass += rows[3 * p + 2];
    ok = ok && mass == (double)K * (double)E * (weighted ? 1.5 : 1.0) + (double)all_added;   // (sums of 1.5 and 1.0: exact)
    if (!ok) { std::printf("%s: FAILED, %lld rows\n", what, (long long)got); ++failures; return; }
    std::printf("%s: ok (%lld rows, %lld distinct in the input)\n", what, (long long)got, (long long)stats[0]);
}

}  // namespace

int main() {
    for (int64_t E : {0, 1, ROW_TILE - 1, ROW_TILE, ROW_TILE + 1, 2 * ROW_TILE + 1})
        for (int K = 1; K <= 3; ++K)
            for (int coalesce = 0; coalesce < 2; ++coalesce)
                call("tile edge", random_rows(E, 97), std::vector<int64_t>(K, E / 3 + (E ? 1 : 0)), coalesce, 0, K == 2);
    call("three nodes", random_rows(50, 3), {3 * ROW_TILE, 7}, 1, 0);
    call("two nodes", random_rows(50, 2), {ROW_TILE + 1}, 1, 0, true);
    call("the widest keys", random_rows(300, ((int64_t)1 << 31) - 1), {100, 0, 750}, 1, 0, false, false);
    call("32 views", random_rows(100, 40), std::vector<int64_t>(32, 30), 1, 0);
    call("no rows, no nodes", random_rows(0, 0), {0, 0}, 1, 0);
    call("no rows, no nodes, not coalesced", random_rows(0, 0), {0}, 0, 0);
    // malformed inputs
    Rows bad = random_rows(100, 40);
    bad.dst[3] = bad.N;
    call("an id past the last node", bad, {10}, 1, REFUSE_RANGE);
    bad.dst[3] = -1;
    call("a negative id", bad, {10}, 0, REFUSE_RANGE);
    Rows none = random_rows(100, 40);
    none.N = 0;
    call("rows without nodes", none, {0}, 1, REFUSE_RANGE);
    call("added rows on one node", random_rows(5, 1), {2}, 1, REFUSE_BAD_ARG);
    call("added rows without nodes", random_rows(0, 0), {1}, 1, REFUSE_BAD_ARG);
    call("33 views", random_rows(100, 40), std::vector<int64_t>(33, 1), 1, REFUSE_TOO_LARGE);
    call("no view", random_rows(100, 40), {}, 1, REFUSE_BAD_ARG);
    call("a negative count", random_rows(100, 40), {3, -1}, 1, REFUSE_BAD_ARG);
    call("2^31 rows in a view", random_rows(100, 40), {((int64_t)1 << 31) - 101}, 1, REFUSE_TOO_LARGE);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
