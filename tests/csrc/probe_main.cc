// The index arithmetic of the linear-probe evaluator (rlap_amd/csrc/rlap_probe.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_probe_cpu.py: for every n_train up to the bound given on the command line (and a few
// large ones), F in {1, 3, 32, 33, 257, 512} and C in {2, 3, 8, 9, 16, 33, 64} it walks the parts, their tiles and chunks, the
// thread maps of the logits and of the gradient and the layouts of the image, the partial sums and the chunk sums through arrays of
// exactly the sizes the library carves, so that an index out of range is an error of the sanitizer and a cell visited twice or
// never one of the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rlap_probe.h"

using namespace rlap;

static int64_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

constexpr int THREADS = 256;

static void check_thread_maps(int64_t F, int64_t C) {
    const int CP = probe::class_pad(C);
    CHECK(CP >= C && (CP == 8 || CP == 16 || CP == 32 || CP == 64) && (CP == probe::MIN_CP || CP / 2 < C), "class_pad(%lld) = %d", (long long)C, CP);
    // the logits: thread (c = tid % CP, rg = tid / CP) owns rows rg + j RG, j < NJ, of the 32 x (CP + 1) tile
    const int NJ = CP / 8, RG = THREADS / CP;
    CHECK(NJ * RG == probe::TILE, "rows of the logits map for CP = %d", CP);
    std::vector<int> z((size_t)(probe::TILE * (CP + 1)), 0);
    for (int tid = 0; tid < THREADS; ++tid)
        for (int j = 0; j < NJ; ++j) ++z[(size_t)((tid / CP + j * RG) * (CP + 1) + tid % CP)];
    for (int i = 0; i < probe::TILE; ++i)
        for (int c = 0; c <= CP; ++c) CHECK(z[(size_t)(i * (CP + 1) + c)] == (c < CP ? 1 : 0), "logit (%d, %d) of CP = %d", i, c, CP);
    // the gradient: thread tid owns columns tid + 256 a, a < KA
    const int KA = F <= THREADS ? 1 : 2;
    std::vector<int> col((size_t)F, 0);
    for (int tid = 0; tid < THREADS; ++tid)
        for (int a = 0; a < KA; ++a)
            if (tid + a * THREADS < F) ++col[(size_t)(tid + a * THREADS)];
    for (int64_t k = 0; k < F; ++k) CHECK(col[(size_t)k] == 1, "column %lld of F = %lld", (long long)k, (long long)F);
    const int64_t LS = probe::image_stride(F);
    CHECK(LS >= F && LS <= F + 1 && LS % 2 == 1, "image stride of %lld", (long long)F);
}

static void check_n(int64_t n, int64_t F, int64_t C, bool elements) {
    const int64_t T = probe::num_tiles(n), Np = probe::padded_rows(n), P = probe::num_parts(n, F, C), nc = spmm::num_chunks(n);
    const int64_t LS = probe::image_stride(F);
    CHECK(T == (n + 31) / 32 && Np == 32 * T && Np >= n && Np < n + 32, "tiles of %lld", (long long)n);
    CHECK(P >= 1 && P <= probe::MAX_PARTS && P <= (nc > 0 ? nc : 1), "parts of %lld: %lld", (long long)n, (long long)P);
    CHECK(probe::part_begin(n, F, C, 0) == 0 && probe::part_end(n, F, C, P - 1) == n, "ends of the parts of %lld", (long long)n);
    std::vector<int> row((size_t)n, 0), chunk((size_t)nc, 0);
    std::vector<float> image(elements ? (size_t)(Np * LS) : 0, 0.0f), partial(elements ? (size_t)(P * C * F) : 0, 0.0f);
    std::vector<double> bchunk((size_t)(nc * C), 0.0);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t rb = probe::part_begin(n, F, C, p), re = probe::part_end(n, F, C, p);
        CHECK(rb < re && rb % spmm::CHUNK == 0 && (re % spmm::CHUNK == 0 || re == n), "part %lld of %lld: [%lld, %lld)", (long long)p, (long long)n, (long long)rb, (long long)re);
        for (int64_t row0 = rb; row0 < re; row0 += probe::TILE) {
            const int nrows = re - row0 < probe::TILE ? (int)(re - row0) : probe::TILE;
            CHECK(row0 + probe::TILE <= Np, "tile at %lld of %lld leaves the image", (long long)row0, (long long)n);
            if (elements)
                for (int64_t j = 0; j < probe::TILE * LS; ++j) image[(size_t)(row0 * LS + j)] += 1.0f;   // the staging of a tile
            for (int i = 0; i < nrows; ++i) ++row[(size_t)(row0 + i)];
            const int64_t next = row0 + probe::TILE;
            if (next % spmm::CHUNK == 0 || next >= re) {
                const int64_t q = row0 / spmm::CHUNK;
                CHECK(q >= 0 && q < nc, "chunk %lld of %lld", (long long)q, (long long)n);
                if (q >= 0 && q < nc) {
                    ++chunk[(size_t)q];
                    for (int64_t c = 0; c < C; ++c) bchunk[(size_t)(q * C + c)] += 1.0;
                    CHECK(spmm::chunk_begin(q) <= row0 && next >= spmm::chunk_end(n, q), "chunk %lld ends early at %lld", (long long)q, (long long)next);
                }
            }
        }
        if (elements)
            for (int64_t c = 0; c < C; ++c)
                for (int64_t k = 0; k < F; ++k) partial[(size_t)((p * C + c) * F + k)] += 1.0f;
    }
    for (int64_t i = 0; i < n; ++i) CHECK(row[(size_t)i] == 1, "row %lld of %lld is visited %d times", (long long)i, (long long)n, row[(size_t)i]);
    for (int64_t q = 0; q < nc; ++q) CHECK(chunk[(size_t)q] == 1, "chunk %lld of %lld is written %d times", (long long)q, (long long)n, chunk[(size_t)q]);
    for (double v : bchunk) CHECK(v == 1.0, "a chunk sum of %lld", (long long)n);
    if (elements) {
        for (float v : image) CHECK(v == 1.0f, "an image cell of (%lld, %lld)", (long long)n, (long long)F);
        for (float v : partial) CHECK(v == 1.0f, "a partial cell of (%lld, %lld, %lld)", (long long)n, (long long)F, (long long)C);
    }
}

int main(int argc, char** argv) {
    const int64_t bound = argc > 1 ? std::atoll(argv[1]) : 600;
    const int64_t Fs[] = {1, 3, 32, 33, 257, 512}, Cs[] = {2, 3, 8, 9, 16, 33, 64};
    for (int64_t F : Fs)
        for (int64_t C : Cs) check_thread_maps(F, C);
    int64_t sizes = 0;
    for (int64_t n = 1; n <= bound; ++n, ++sizes)
        for (int64_t F : Fs)
            for (int64_t C : Cs) check_n(n, F, C, (F == 3 || F == 33) && (C == 3 || C == 64));
    const int64_t large[] = {2708, 16383, 16384, 16385, 16640, 90941, 169343, ((int64_t)1 << 31) - 1};
    for (int64_t n : large) {
        const int64_t P = probe::num_parts(n, 1, 2);
        CHECK(P == (n > 64 * 256 - 256 ? 64 : (n + 255) / 256) || P == 64, "parts of %lld: %lld", (long long)n, (long long)P);
        if (n < (int64_t)1 << 20) check_n(n, 3, 3, true);
        int64_t prev = 0;
        for (int64_t p = 0; p < P; ++p) {
            const int64_t b = probe::part_begin(n, 1, 2, p), e = probe::part_end(n, 1, 2, p);
            CHECK(b == prev && e > b, "part %lld of %lld", (long long)p, (long long)n);
            prev = e;
        }
        CHECK(prev == n, "the parts of %lld end at %lld", (long long)n, (long long)prev);
    }
    // the scores of a few matrices: a label absent from both sides is left out of the macro mean
    const int64_t conf[9] = {2, 0, 0, 1, 3, 0, 0, 0, 0};
    double micro, macro, acc;
    probe::scores_of(conf, 3, 6, &micro, &macro, &acc);
    CHECK(micro == 5.0 / 6.0 && acc == micro && macro == (4.0 / 5.0 + 6.0 / 7.0) / 2.0, "scores %g %g %g", micro, macro, acc);
    std::printf("%lld sizes, %lld failures\n", (long long)sizes, (long long)failures);
    return failures ? 1 : 0;
}
