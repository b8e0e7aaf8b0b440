// The feature plan's mirror (tests/csrc/featlin_mirror.cc around rlap_amd/csrc/rlap_featlin.h) in a stand-alone program, built with
// g++ -fsanitize=address,undefined by tests/test_featlin_cpu.py.  Every buffer has exactly the stated size, so a read or write
// outside it stops the program.  Covered: builds and both products over list lengths around the chunk, both types, K up to 32; a
// truncated buffer (refused); offsets, ids and directory entries out of range (clamped: wrong numbers, no access out of range).
// Prints "<n> cases, <f> failures".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "featlin_mirror.cc"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static uint64_t state = 0x9E3779B97F4A7C15ull;
static double next01() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (double)(state >> 11) / 9007199254740992.0; }

template <class T>
static void run_case(int64_t N, int64_t Fin, double density, int64_t K, int64_t F, int dirs) {
    const int f32 = sizeof(T) == 4;
    std::vector<T> x((size_t)(N * Fin));
    for (auto& v : x) v = next01() < density ? (T)(next01() - 0.5) : (T)0;
    if (N * Fin > 3) { x[1] = (T)-0.0; x[2] = (T)NAN; }
    const int64_t nnz = featlin_count(x.data(), f32, N, Fin);
    int64_t lay[7];
    featlin_layout(N, Fin, nnz, dirs & 1, dirs & 2, lay);
    std::vector<uint8_t> buf((size_t)lay[6]);
    int64_t desc[D_WORDS], info[6];
    CHECK(featlin_build(x.data(), f32, N, Fin, nnz + 1, dirs & 1, dirs & 2, buf.data(), lay[6], desc, info) == 3 && desc[D_BYTES] == 0);
    CHECK(featlin_build(x.data(), f32, N, Fin, nnz, dirs & 1, dirs & 2, buf.data(), lay[6] - 1, desc, info) == 3);
    CHECK(featlin_build(x.data(), f32, N, Fin, nnz, dirs & 1, dirs & 2, buf.data(), lay[6], desc, info) == 0);
    std::vector<uint8_t> keep((size_t)(K * Fin));
    for (auto& b : keep) b = next01() < 0.7 ? 1 : 0;
    std::vector<T> w((size_t)(Fin * F)), y((size_t)(K * N * F)), g((size_t)(K * N * F)), dw((size_t)(Fin * F));
    for (auto& v : w) v = (T)(next01() - 0.5);
    for (auto& v : g) v = (T)(next01() - 0.5);
    for (int t = 0; t < 2; ++t) {
        const void* in = t ? (const void*)g.data() : (const void*)w.data();
        void* out = t ? (void*)dw.data() : (void*)y.data();
        const bool has = (dirs & (t ? 2 : 1)) != 0;
        CHECK(featlin_apply(buf.data(), lay[6], desc, t, f32, in, keep.data(), K, F, out) == (has ? 0 : 3));
        CHECK(featlin_apply(buf.data(), lay[6], desc, t, f32, in, nullptr, K, F, out) == (has && K == 1 ? 0 : 3));
        CHECK(featlin_apply(buf.data(), lay[6], desc, t, f32, in, keep.data(), 0, F, out) == 3);
        CHECK(featlin_apply(buf.data(), lay[6], desc, t, f32, in, keep.data(), 33, F, out) == 3);
        if (!has) continue;
        // a truncated buffer: a copy of exactly the shorter size, refused before anything is read
        for (int64_t cut : {(int64_t)1, (int64_t)16, (int64_t)256, lay[6] / 2}) {
            if (cut >= lay[6]) continue;
            std::vector<uint8_t> shorter(buf.begin(), buf.end() - cut);
            const int rc = featlin_apply(shorter.data(), lay[6] - cut, desc, t, f32, in, keep.data(), K, F, out);
            CHECK(rc == 3 || rc == 0);   // (a cut inside the padding behind the last part leaves every part whole)
            if (nnz > 0 && cut >= 256 && (dirs != 3 || t == 1)) CHECK(rc == 3);   // (the records of the last direction are the tail)
        }
        // offsets, ids and directory entries out of range: clamped
        std::vector<uint8_t> bad(buf);
        const int64_t slots = t ? Fin : N;
        int64_t* off = reinterpret_cast<int64_t*>(bad.data() + desc[t ? D_OFF_T : D_OFF_F]);
        plan::Record* rec = reinterpret_cast<plan::Record*>(bad.data() + desc[t ? D_REC_T : D_REC_F]);
        plan::ChunkRef* dir = reinterpret_cast<plan::ChunkRef*>(bad.data() + desc[t ? D_DIR_T : D_DIR_F]);
        for (int64_t s = 0; s <= slots; s += 3) off[s] = (s % 2) ? -(int64_t)1e15 : (int64_t)1e15;
        if (slots > 1) off[1] = nnz + 1;
        for (int64_t e = 0; e < nnz; e += 5) rec[e].id = (e % 2) ? INT32_MAX : INT32_MIN;
        for (int64_t q = 0; q < desc[t ? D_CHUNKS_T : D_CHUNKS_F]; ++q) { dir[q].slot = (q % 2) ? -5 : (int64_t)1e15; dir[q].k = -q; }
        CHECK(featlin_apply(bad.data(), lay[6], desc, t, f32, in, keep.data(), K, F, out) == 0);
        CHECK(featlin_dir_first(bad.data(), lay[6], desc, t, slots / 2) >= 0);
    }
}

int main() {
    long long cases = 0;
    const int64_t shapes[][2] = {{1, 1}, {3, 7}, {2, 520}, {520, 2}, {300, 300}, {65, 257}};
    for (const auto& s : shapes)
        for (double density : {0.0, 0.05, 1.0})
            for (int dirs : {1, 2, 3})
                for (int64_t K : {(int64_t)1, (int64_t)3, (int64_t)9}) {
                    if (s[0] * s[1] > 50000 && (K == 3 || density == 0.05) && dirs != 3) continue;
                    run_case<float>(s[0], s[1], density, K, 3, dirs);
                    run_case<double>(s[0], s[1], density, K, 2, dirs);
                    cases += 2;
                }
    run_case<float>(4, 5, 0.5, 32, 1, 3);
    ++cases;
    int64_t lay[7];
    featlin_layout(5, 9, 1000, 1, 1, lay);
    for (int k = 0; k < 7; ++k) CHECK(lay[k] >= 0 && lay[k] % 256 == 0);
    featlin_layout(5, 9, 1000, 0, 1, lay);
    CHECK(lay[0] == -1 && lay[2] == -1 && lay[4] == -1 && lay[1] == 0);
    std::printf("%lld cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
