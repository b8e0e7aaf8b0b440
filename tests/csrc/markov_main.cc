// markov_main.cc -- the Markov diffusion mirror (markov_mirror.cc) as a stand-alone program with its own main, for a build with
// -fsanitize=address,undefined (tests/test_markov_cpu.py): closed forms on one loop row, two nodes and a star, both parities of the
// order, an id without edges, a subset of the source tiles on a path of 200 nodes, then malformed inputs, which the call refuses.
// Prints one line per call; exits 0 when every call answered as expected.
#include <cmath>
#include <cstdio>
#include <vector>

#include "markov_mirror.cc"

namespace {

int failures = 0;

struct Out { int64_t rows; std::vector<double> raw, norm; };

Out run(const std::vector<double>& sc, int weighted, int loop, int zero_ok, double alpha, int order, double eps,
        const std::vector<int64_t>* tiles = nullptr) {
    Out o;
    o.rows = markov_run(sc.data(), (int64_t)sc.size() / 3, weighted, loop, zero_ok, alpha, order, eps, tiles ? tiles->data() : nullptr,
                        tiles ? (int64_t)tiles->size() : -1);
    if (o.rows > 0) {
        o.raw.resize(3 * (size_t)o.rows); o.norm.resize(3 * (size_t)o.rows);
        markov_fetch(o.raw.data(), o.norm.data());
    }
    return o;
}

void expect(const char* what, bool ok) {
    std::printf("%s: %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) ++failures;
}

bool near(double a, double b) { return std::fabs(a - b) <= 1e-14 * std::fabs(b); }

// sum_{k=0..D} beta^k
double geo(double beta, int D) { double s = 0.0, p = 1.0; for (int k = 0; k <= D; ++k) { s += p; p *= beta; } return s; }

std::vector<double> path_rows(int64_t n) {   // grouped by column: (c - 1, c), (c + 1, c)
    std::vector<double> sc;
    for (int64_t c = 0; c < n; ++c) {
        if (c > 0) { sc.push_back((double)(c - 1)); sc.push_back((double)c); sc.push_back(1.0 + 0.25 * (double)((c - 1) % 3)); }
        if (c + 1 < n) { sc.push_back((double)(c + 1)); sc.push_back((double)c); sc.push_back(1.0 + 0.25 * (double)(c % 3)); }
    }
    return sc;
}

}  // namespace

int main() {
    // one loop row (7, 7, w): Â = 1, M = alpha + geo / D, for every order parity
    for (int D : {1, 2, 3, 16}) {
        const Out o = run({7.0, 7.0, 2.5}, 1, 0, 0, 0.2, D, 1e-4);
        expect("one loop row", o.rows == 1 && o.raw[0] == 7.0 && o.raw[1] == 7.0 && near(o.raw[2], 0.2 + geo(0.8, D) / D) && near(o.norm[2], 1.0));
    }
    // two nodes, one edge, no loop: Â = [[0,1],[1,0]]: even powers on the diagonal, odd ones off it
    {
        const int D = 3;
        const double b = 0.75;
        const Out o = run({1.0, 0.0, 3.0, 0.0, 1.0, 3.0}, 1, 0, 0, 0.25, D, 1e-6);
        const double off = 0.25 + (1.0 + b * b) / D, dia = (b + b * b * b) / D;
        expect("two nodes", o.rows == 4 && near(o.raw[2], dia) && near(o.raw[5], off) && o.raw[5] == o.raw[8] && near(o.raw[11], dia));
    }
    // an id without edges: no row without the loop, alpha + geo / D with it
    {
        const std::vector<double> sc = {1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 5.0, 5.0, 0.0};
        const Out a = run(sc, 1, 0, 1, 0.2, 2, 1e-4), b = run(sc, 1, 1, 1, 0.2, 2, 1e-4);
        bool no5 = true;
        for (int64_t r = 0; r < a.rows; ++r) no5 = no5 && a.raw[3 * r] != 5.0;
        expect("no edges, no loop", a.rows == 4 && no5);
        expect("no edges, loop", b.rows == 5 && b.raw[12] == 5.0 && b.raw[13] == 5.0 && near(b.raw[14], 0.2 + geo(0.8, 2) / 2));
        expect("a zero weight is refused without the flag", run(sc, 1, 0, 0, 0.2, 2, 1e-4).rows == -MK_BAD_ARG);
    }
    // a star of 70 nodes (two tiles), unit weights: exactly symmetric, alpha = 0 and 1
    for (double alpha : {0.0, 0.2, 1.0}) {
        std::vector<double> sc;
        for (int64_t l = 1; l < 70; ++l) { sc.push_back((double)l); sc.push_back(0.0); sc.push_back(1.0); }
        for (int64_t l = 1; l < 70; ++l) { sc.push_back(0.0); sc.push_back((double)l); sc.push_back(1.0); }
        const Out o = run(sc, 0, 1, 0, alpha, 16, 1e-6);
        bool sym = o.rows > 0;
        for (int64_t r = 0; r < o.rows && sym; ++r) {
            bool found = false;
            for (int64_t q = 0; q < o.rows; ++q)
                if (o.raw[3 * q] == o.raw[3 * r + 1] && o.raw[3 * q + 1] == o.raw[3 * r]) found = o.raw[3 * q + 2] == o.raw[3 * r + 2] && o.norm[3 * q + 2] == o.norm[3 * r + 2];
            sym = found;
        }
        expect("star of 70", sym);
    }
    // a subset of the tiles of a path of 200 nodes: the rows of the whole run whose smaller id lies in the tile
    {
        const std::vector<double> sc = path_rows(200);
        const Out all = run(sc, 1, 1, 0, 0.2, 16, 1e-3);
        const std::vector<int64_t> tiles = {1, 3};
        const Out part = run(sc, 1, 1, 0, 0.2, 16, 1e-3, &tiles);
        std::vector<double> want;
        for (int64_t r = 0; r < all.rows; ++r) {
            const int64_t lo = (int64_t)std::min(all.raw[3 * r], all.raw[3 * r + 1]);
            if ((lo >= 64 && lo < 128) || lo >= 192) want.insert(want.end(), all.raw.begin() + 3 * r, all.raw.begin() + 3 * r + 3);
        }
        expect("tile subset", part.rows > 0 && part.raw == want && all.rows < 200 * 200);
    }
    // refusals
    expect("alpha > 1", run({0.0, 0.0, 1.0}, 1, 0, 0, 1.5, 2, 1e-4).rows == -MK_BAD_ARG);
    expect("order 0", run({0.0, 0.0, 1.0}, 1, 0, 0, 0.2, 0, 1e-4).rows == -MK_BAD_ARG);
    expect("order past the cap", run({0.0, 0.0, 1.0}, 1, 0, 0, 0.2, rlap::markov::MAX_ORDER + 1, 1e-4).rows == -MK_BAD_ARG);
    expect("eps 0", run({0.0, 0.0, 1.0}, 1, 0, 0, 0.2, 2, 0.0).rows == -MK_BAD_ARG);
    expect("a row id without a column", run({1.0, 0.0, 1.0}, 1, 0, 0, 0.2, 2, 1e-4).rows == -MK_NOT_SYMMETRIC);
    expect("a column in two runs", run({1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 0.0, 1.0}, 1, 0, 0, 0.2, 2, 1e-4).rows == -MK_NOT_GROUPED);
    expect("no rows", run({}, 1, 1, 0, 0.2, 2, 1e-4).rows == 0);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
