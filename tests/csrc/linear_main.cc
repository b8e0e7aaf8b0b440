// The index arithmetic of the fused dense layer (rlap_amd/csrc/rlap_linear.h) and its mirror as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_linear_cpu.py.  It walks, through arrays of exactly the sizes the library carves or the
// caller owns, so that an index out of range is an error of the sanitizer and a cell visited twice or never one of the program:
//   * for every (Fin, Fout) in [1, 512]^2 and a sweep of M: the parts (contiguous, multiples of 32, covering the padded rows);
//   * for every count of column tiles and a sweep of M and widths: the work map of the product kernels (every tile owned by exactly
//     one wave, the instance holds its tiles), the staging of the weight slab, the guarded loads of the A operand on both lane
//     paths and the guarded stores;
//   * for every pair of tile counts: the work map of the weight gradient (every tile of every part stored once), the staged slabs
//     and the operands read from them, the guarded fetches on both lane paths;
//   * the mirror itself over the edge shapes, every activation and both layouts.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "linear_mirror.cc"

static int64_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

constexpr int THREADS = 256, A_COLS = 64;   // rlap_linear.hip's LIN_THREADS and LIN_A_COLS

// rlap_linear.hip's lin_load4 on an array of exactly M F floats: which of the four elements are read (the others are zeros)
static void load4(const std::vector<float>& p, bool vec, int64_t row, int col, int64_t M, int F, int* reads) {
    if (row >= M) return;
    if (vec) {
        CHECK(F % 4 == 0 && col % 4 == 0, "a 16-byte load at width %d, column %d", F, col);
        if (col < F) {
            float s = 0.0f;
            for (int e = 0; e < 4; ++e) s += p[(size_t)(row * F + col + e)];
            *reads += 4 + (s != 0.0f);
        }
    } else {
        for (int e = 0; e < 4; ++e)
            if (col + e < F) *reads += 1 + (p[(size_t)(row * F + col + e)] != 0.0f);
    }
}

static void check_parts(int64_t M, int64_t Fin, int64_t Fout) {
    const int64_t T = linear::num_tiles(M), Mp = linear::padded_rows(M), P = linear::num_parts(M, Fin, Fout);
    CHECK(P >= 1 && P <= T && P <= linear::MAX_PARTS, "parts of (%lld, %lld, %lld): %lld", (long long)M, (long long)Fin, (long long)Fout, (long long)P);
    CHECK(linear::part_begin(M, Fin, Fout, 0) == 0 && linear::part_begin(M, Fin, Fout, P) == Mp, "ends of the parts of %lld", (long long)M);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t r0 = linear::part_begin(M, Fin, Fout, p), r1 = linear::part_begin(M, Fin, Fout, p + 1);
        CHECK(r0 < r1 && r0 % 32 == 0 && r1 % 32 == 0, "part %lld of (%lld, %lld, %lld)", (long long)p, (long long)M, (long long)Fin, (long long)Fout);
    }
}

// the product kernel of (M, K) x (K, C)
static void check_product(int64_t M, int K, int C) {
    const int nct = linear::feature_tiles(C), Kp = linear::padded_features(K), Cp = linear::padded_features(C);
    const int CW = linear::col_waves(nct), RT = linear::row_tiles(nct), NCT = linear::product_instance(nct);
    const int64_t T = linear::num_tiles(M), G = linear::product_groups(M, nct);
    CHECK(CW * RT == linear::WAVES && NCT >= 1 && NCT <= 4 && CW * NCT >= nct && CW * (NCT - 1) < nct, "instance (%d, %d) of %d tiles", CW, NCT, nct);
    CHECK(G * RT >= T && (G - 1) * RT < T, "groups of %lld", (long long)M);
    // the slab of the weight image: float4 tid + 256 j, j < nct, of 8 Cp
    std::vector<int> slab((size_t)(8 * Cp), 0);
    for (int tid = 0; tid < THREADS; ++tid)
        for (int j = 0; j < CW * NCT; ++j)
            if (j < nct) ++slab[(size_t)(tid + j * THREADS)];
    for (size_t e = 0; e < slab.size(); ++e) CHECK(slab[e] == 1, "float4 %zu of the slab at %d tiles staged %d times", e, nct, slab[e]);
    std::vector<float> lds((size_t)(32 * Cp), 0.0f), A((size_t)(M * K), 0.0f);
    std::vector<int> out((size_t)(M * C), 0), owner((size_t)(T * nct), 0);
    for (int64_t g = 0; g < G; ++g)
        for (int w = 0; w < linear::WAVES; ++w) {
            const int64_t tile = linear::wave_row_tile(g, w, nct);
            CHECK(linear::wave_col_tile(w, NCT, nct) >= nct, "wave %d owns a tile its instance %d does not hold", w, NCT);
            for (int vec = 0; vec < 2; ++vec) {
                if (vec && K % 4 != 0) continue;
                int reads = 0;
                for (int l0 = 0; l0 < Kp; l0 += 32)
                    for (int c = 0; c < 32; ++c)
                        for (int q = 0; q < 8; ++q) load4(A, vec != 0, tile * 32 + c, l0 + 4 * q, M, K, &reads);
                const int64_t live = tile * 32 >= M ? 0 : (M - tile * 32 < 32 ? M - tile * 32 : 32);
                CHECK(reads == live * K, "wave (%lld, %d) reads %d of %lld elements of A", (long long)g, w, reads, (long long)(live * K));
            }
            for (int j = 0; j < NCT; ++j) {
                const int ct = linear::wave_col_tile(w, j, nct);
                if (ct >= nct) continue;
                if (tile < T) ++owner[(size_t)(tile * nct + ct)];
                for (int h = 0; h < 2; ++h)
                    for (int c = 0; c < 32; ++c) {
                        float s = 0.0f;
                        for (int st = 0; st < 16; ++st) s += lds[(size_t)(h * Cp + c + 2 * st * Cp + ct * 32)];
                        CHECK(s == 0.0f, "the slab");
                        const int col = ct * 32 + c;
                        if (col >= C) continue;
                        for (int r = 0; r < 16; ++r) {
                            const int64_t orow = tile * 32 + linear::reg_row(r, h);
                            if (orow < M) ++out[(size_t)(orow * C + col)];
                        }
                    }
            }
        }
    for (size_t e = 0; e < owner.size(); ++e) CHECK(owner[e] == 1, "tile %zu of (%lld, %d) owned %d times", e, (long long)M, C, owner[e]);
    for (size_t e = 0; e < out.size(); ++e) CHECK(out[e] == 1, "element %zu of (%lld, %d) stored %d times", e, (long long)M, C, out[e]);
}

// the weight gradient of (M, Fin, Fout)
static void check_cross(int64_t M, int Fin, int Fout) {
    const int nfi = linear::feature_tiles(Fin), nfo = linear::feature_tiles(Fout), Finp = 32 * nfi, Foutp = 32 * nfo;
    const int nsi = linear::super_tiles(Fin), nso = linear::super_tiles(Fout), rg = linear::row_groups(Fout), groups = linear::pair_groups(Fin, Fout);
    const int NW = linear::cross_instance(nfo);
    const int64_t P = linear::num_parts(M, Fin, Fout);
    CHECK(groups == nsi * rg && rg * 4 >= nso && (rg - 1) * 4 < nso, "groups of (%d, %d)", Fin, Fout);
    CHECK((NW == 1 || NW == 2 || NW == 4) && NW >= (nso < 4 ? nso : 4), "cross instance %d of %d", NW, Fout);
    if (!(NW == 1 || NW == 2 || NW == 4)) return;
    const int BW = 64 * NW, AV = A_COLS / 4, BV = BW / 4;
    std::vector<float> X((size_t)(M * Fin), 0.0f), Tt((size_t)(M * Fout), 0.0f);
    std::vector<int> cells((size_t)(P * Finp * Foutp), 0);
    for (int64_t block = 0; block < P * groups; ++block) {
        const int grp = (int)(block % groups), part = (int)(block / groups);
        int I, J0;
        linear::group_of(grp, rg, &I, &J0);
        CHECK(0 <= I && I < nsi && 0 <= J0 && J0 < nso && J0 % 4 == 0, "group %d of (%d, %d)", grp, Fin, Fout);
        const int64_t r0 = linear::part_begin(M, Fin, Fout, part);
        const bool vec = Fin % 4 == 0 && Fout % 4 == 0;
        // the staged slabs of the part's first rows: 1 an element of the arrays or a zero behind them
        std::vector<int8_t> sa((size_t)(32 * A_COLS), 0), sb((size_t)(32 * BW), 0);
        int reads = 0;
        for (int tid = 0; tid < THREADS; ++tid) {
            for (int j = 0; j < 2; ++j) {
                const int v = tid + THREADS * j, col = A_COLS * I + 4 * (v % AV), row = v / AV;
                CHECK(row < 32 && 4 * v == row * A_COLS + (col - A_COLS * I), "the slab of x is row-major");
                load4(X, vec, r0 + row, col, M, Fin, &reads);
                for (int e = 0; e < 4; ++e) ++sa[(size_t)(4 * v + e)];
            }
            for (int j = 0; j < 2 * NW; ++j) {
                const int v = tid + THREADS * j, col = A_COLS * J0 + 4 * (v % BV), row = v / BV;
                CHECK(row < 32 && 4 * v == row * BW + (col - A_COLS * J0), "the slab of t is row-major");
                load4(Tt, vec, r0 + row, col, M, Fout, &reads);
                for (int e = 0; e < 4; ++e) ++sb[(size_t)(4 * v + e)];
            }
        }
        for (size_t e = 0; e < sa.size(); ++e) CHECK(sa[e] == 1, "float %zu of the slab of x staged %d times", e, (int)sa[e]);
        for (size_t e = 0; e < sb.size(); ++e) CHECK(sb[e] == 1, "float %zu of the slab of t staged %d times", e, (int)sb[e]);
        for (int wave = 0; wave < 4; ++wave) {
            if (!(wave < NW && linear::wave_active(J0, wave, nso))) continue;
            const int J = J0 + wave;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b) {
                    const int ka = linear::tile_of(I, a, nfi) * 32 - A_COLS * I, kb = linear::tile_of(J, b, nfo) * 32 - A_COLS * J0;
                    CHECK(ka >= 0 && ka + 32 <= A_COLS && kb >= 0 && kb + 32 <= BW, "operand columns (%d, %d)", ka, kb);
                    int8_t s = 0;
                    for (int st = 0; st < 16; ++st)
                        for (int h = 0; h < 2; ++h) s |= (int8_t)(sa[(size_t)(h * A_COLS + 31 + 2 * st * A_COLS + ka)] | sb[(size_t)(h * BW + 31 + 2 * st * BW + kb)]);
                    CHECK(s == 1, "the operands");
                    if (!linear::tile_stored(I, J, a, b, nfi, nfo)) continue;
                    const int k0 = (2 * I + a) * 32, l0 = (2 * J + b) * 32;
                    for (int h = 0; h < 2; ++h)
                        for (int r = 0; r < 16; ++r)
                            for (int c = 0; c < 32; ++c) ++cells[(size_t)(((int64_t)part * Finp + k0 + linear::reg_row(r, h)) * Foutp + l0 + c)];
                }
        }
    }
    for (size_t e = 0; e < cells.size(); ++e) CHECK(cells[e] == 1, "cell %zu of (%lld, %d, %d) written %d times", e, (long long)M, Fin, Fout, cells[e]);
}

// the mirror on a small case: finite results, and the out_in call on W^T gives the bits of the plain call
static void check_mirror(int64_t M, int Fin, int Fout) {
    std::vector<float> x((size_t)(M * Fin)), w((size_t)(Fin * Fout)), wt((size_t)(Fin * Fout)), b((size_t)Fout), gy((size_t)(M * Fout));
    for (size_t e = 0; e < x.size(); ++e) x[e] = (float)((int)(e * 7 % 13) - 6) / 8.0f;
    for (int k = 0; k < Fin; ++k)
        for (int o = 0; o < Fout; ++o) wt[(size_t)(o * Fin + k)] = w[(size_t)(k * Fout + o)] = (float)((k * 5 + o * 3) % 11 - 5) / 16.0f;
    for (int o = 0; o < Fout; ++o) b[(size_t)o] = (float)(o % 5 - 2) / 4.0f;
    for (size_t e = 0; e < gy.size(); ++e) gy[e] = (float)((int)(e * 3 % 7) - 3) / 4.0f;
    for (int act = 0; act < 3; ++act) {
        std::vector<float> y((size_t)(M * Fout)), y2(y.size()), gx(x.size()), gx2(x.size()), gw(w.size()), gw2(w.size()), gb((size_t)Fout), gb2((size_t)Fout);
        CHECK(lin_mirror(x.data(), w.data(), b.data(), M, Fin, Fout, act, 0.75, 0, 3, 0, y.data()) == 0, "the mirror");
        CHECK(lin_mirror(x.data(), wt.data(), b.data(), M, Fin, Fout, act, 0.75, linear::WEIGHT_OUT_IN, 2, 1, y2.data()) == 0, "the mirror");
        CHECK(std::memcmp(y.data(), y2.data(), y.size() * 4) == 0, "y of both layouts at (%lld, %d, %d)", (long long)M, Fin, Fout);
        CHECK(lin_mirror_backward(x.data(), w.data(), y.data(), gy.data(), M, Fin, Fout, act, 0.75, 0, 3, 0, gx.data(), gw.data(), gb.data()) == 0, "the mirror");
        CHECK(lin_mirror_backward(x.data(), wt.data(), y.data(), gy.data(), M, Fin, Fout, act, 0.75, linear::WEIGHT_OUT_IN, 2, 1, gx2.data(), gw2.data(), gb2.data()) == 0, "the mirror");
        CHECK(std::memcmp(gx.data(), gx2.data(), gx.size() * 4) == 0 && std::memcmp(gb.data(), gb2.data(), gb.size() * 4) == 0, "gx, gb of both layouts");
        for (int k = 0; k < Fin; ++k)
            for (int o = 0; o < Fout; ++o) CHECK(std::memcmp(&gw[(size_t)(k * Fout + o)], &gw2[(size_t)(o * Fin + k)], 4) == 0, "gw of both layouts");
        CHECK(lin_mirror_backward(x.data(), w.data(), y.data(), gy.data(), M, Fin, Fout, act, 0.75, 0, 1, 0, nullptr, nullptr, nullptr) == 0, "no output");
    }
}

int main() {
    const int64_t ms[] = {1, 31, 32, 33, 127, 128, 129, 300, 2049, 2708, 4245, 169343, 12582912, ((int64_t)1 << 31) - 1};
    for (int64_t Fin = 1; Fin <= linear::MAX_F; ++Fin)
        for (int64_t Fout = 1; Fout <= linear::MAX_F; ++Fout)
            for (int64_t M : ms) check_parts(M, Fin, Fout);
    const int widths[] = {1, 2, 3, 4, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 256, 257, 288, 320, 352, 384, 416, 448, 480, 512};
    const int64_t small[] = {1, 31, 32, 33, 65, 127, 128, 129, 161};
    for (int C : widths)
        for (int64_t M : small)
            for (int K : {1, 3, 4, 33, 64}) check_product(M, K, C);
    check_product(300, 512, 512);
    for (int nfi = 1; nfi <= 16; ++nfi)
        for (int nfo = 1; nfo <= 16; ++nfo)
            for (int64_t M : {(int64_t)1, (int64_t)33, (int64_t)129}) {
                check_cross(M, 32 * nfi, 32 * nfo);                  // the vector lane path
                check_cross(M, 32 * nfi - 31, 32 * nfo - 29);        // the scalar one, the narrowest widths of these tile counts
            }
    check_cross(2049, 33, 65);
    const int edge[] = {1, 2, 3, 31, 32, 33, 65};
    for (int Fin : edge)
        for (int Fout : edge)
            for (int64_t M : {(int64_t)1, (int64_t)33, (int64_t)257}) check_mirror(M, Fin, Fout);
    check_mirror(40, 129, 257);
    CHECK(linear::product_instance(0) == 0 && linear::product_instance(17) == 0 && linear::cross_instance(0) == 0 && linear::cross_instance(17) == 0,
          "no instance outside 1 .. 16 tiles");
    CHECK(linear::alpha_ok(1.0) && linear::alpha_ok(1e-300) && linear::alpha_ok(1e300) && !linear::alpha_ok(0.0) && !linear::alpha_ok(-1.0) &&
              !linear::alpha_ok((double)NAN) && !linear::alpha_ok((double)INFINITY), "alpha");
    CHECK(linear::flags_ok(0) && linear::flags_ok(1) && !linear::flags_ok(2) && !linear::flags_ok(-1) && linear::act_ok(0) && linear::act_ok(2) &&
              !linear::act_ok(3) && !linear::act_ok(-1), "flags and activations");
    CHECK(linear::vec_ok(64, 0) && linear::vec_ok(4, 16) && !linear::vec_ok(64, 4) && !linear::vec_ok(65, 0) && !linear::vec_ok(2, 0), "the lane path");
    std::printf("%lld failures\n", (long long)failures);
    return failures ? 1 : 0;
}
