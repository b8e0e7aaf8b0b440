// The index arithmetic of the fused graph-to-local losses (rlap_amd/csrc/rlap_g2l.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_g2l_cpu.py: for every N up to the bound given on the command line and G in
// {1, 2, 31, 32, 33, 65, N, N + 3} it walks the node tiles, the graph tiles and the parts, the node -> graph map over tables with
// empty graphs at the front, in the middle and at the end, the register-to-row map, the workgroup maps of the three main kernels
// and the row blocks of the vector kernels (for every F from 1 to 512: the instance of the backward kernels that the launchers
// choose and the rows of a vector block), and the arena carve-up through arrays of exactly the carved sizes, so that an index out
// of range is an error of the sanitizer and a cell visited twice or never one of the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rlap_g2l.h"

using namespace rlap;

static int64_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)
#define LL(x) ((long long)(x))

static void check_reg_rows() {
    int seen[32];
    std::memset(seen, 0, sizeof seen);
    for (int hf = 0; hf < 2; ++hf)
        for (int r = 0; r < 16; ++r) {
            const int row = g2l::reg_row(r, hf);
            CHECK(row >= 0 && row < 32, "reg_row(%d, %d) = %d", r, hf, row);
            CHECK(row == g2l::reg_row(r, 0) + 4 * hf, "half offset of register %d", r);
            if (row >= 0 && row < 32) ++seen[row];
        }
    for (int i = 0; i < 32; ++i) CHECK(seen[i] == 1, "row %d is held %d times", i, seen[i]);
}

// a table of G graphs over N nodes with empty graphs at the front, in the middle and at the end where G allows them
static std::vector<int64_t> make_table(int64_t N, int64_t G, int variant) {
    std::vector<int64_t> t(1, 0);
    if (G == 1) { t.push_back(N); return t; }
    const int64_t front = G >= 4 ? 1 : 0, back = G >= 4 ? 1 : 0, middle = G >= 5 ? 1 : 0;
    const int64_t live = G - front - back - middle;   // the graphs that share the nodes; the others are empty
    for (int64_t e = 0; e < front; ++e) t.push_back(0);
    for (int64_t l = 0; l < live; ++l) {
        const int64_t end = variant == 0 ? N * (l + 1) / live : N;   // variant 0: near-equal cuts; 1: everything in the first live graph
        t.push_back(end);
        if (middle && l == (live - 1) / 2) t.push_back(end);
    }
    for (int64_t e = 0; e < back; ++e) t.push_back(N);
    return t;
}

static void check_map(int64_t N, int64_t G) {
    for (int variant = 0; variant < 2; ++variant) {
        const std::vector<int64_t> t = make_table(N, G, variant);
        CHECK((int64_t)t.size() == G + 1 && t[0] == 0 && t[(size_t)G] == N, "table of (%lld, %lld)", LL(N), LL(G));
        for (int64_t j = 0; j < G; ++j) CHECK(t[(size_t)j] <= t[(size_t)j + 1], "table of (%lld, %lld) decreases", LL(N), LL(G));
        std::vector<int64_t> count((size_t)G, 0);
        for (int64_t i = 0; i < N; ++i) {
            const int64_t j = g2l::graph_of(t.data(), G, N, i);
            CHECK(j >= 0 && j < G, "graph_of(%lld) = %lld of %lld", LL(i), LL(j), LL(G));
            if (j < 0 || j >= G) continue;
            CHECK(t[(size_t)j] <= i && i < t[(size_t)j + 1], "node %lld of (%lld, %lld) mapped to graph %lld", LL(i), LL(N), LL(G), LL(j));
            ++count[(size_t)j];
        }
        for (int64_t j = 0; j < G; ++j) CHECK(count[(size_t)j] == t[(size_t)j + 1] - t[(size_t)j], "graph %lld of (%lld, %lld)", LL(j), LL(N), LL(G));
    }
    // a table that is not well formed: the map stays in [0, G)
    std::vector<int64_t> bad((size_t)(G + 1));
    for (int64_t j = 0; j <= G; ++j) bad[(size_t)j] = (j % 3 == 0 ? -5 : (j % 3 == 1 ? (int64_t)1 << 40 : N / 2));
    for (int64_t i = 0; i < N; ++i) {
        const int64_t j = g2l::graph_of(bad.data(), G, N, i);
        CHECK(j >= 0 && j < G, "graph_of on a malformed table: %lld", LL(j));
    }
}

// the workgroup map of a main kernel: `owners` rows own, `streams` rows stream in `parts` parts; every (part, owner row) cell once,
// every stream row once per owner
static void check_main(int64_t owners, int64_t streams, int64_t parts, int64_t N, int64_t G, int64_t F, bool node_parts) {
    const int64_t To = g2l::num_tiles(owners), Ts = g2l::num_tiles(streams), RB = g2l::row_blocks(owners), Op = g2l::padded_rows(owners);
    std::vector<int> cell((size_t)(parts * Op), 0);
    std::vector<int> met((size_t)g2l::padded_rows(streams), 0);
    for (int64_t block = 0; block < RB * parts; ++block) {
        const int64_t blk = block % RB, part = block / RB;
        const int64_t tb = node_parts ? g2l::part_begin(N, G, F, part) : 0, te = node_parts ? g2l::part_begin(N, G, F, part + 1) : Ts;
        CHECK(tb < te && te <= Ts, "part %lld of (%lld, %lld)", LL(part), LL(N), LL(G));
        if (blk == 0)
            for (int64_t t = tb; t < te; ++t)
                for (int r = 0; r < 16; ++r)
                    for (int hf = 0; hf < 2; ++hf) ++met[(size_t)(t * g2l::TILE + g2l::reg_row(r, hf))];
        for (int wave = 0; wave < g2l::BLOCK_TILES; ++wave) {
            const int64_t ot = blk * g2l::BLOCK_TILES + wave;
            if (ot >= To) continue;
            for (int c = 0; c < 32; ++c) ++cell[(size_t)(part * Op + ot * g2l::TILE + c)];
        }
    }
    for (size_t e = 0; e < cell.size(); ++e) CHECK(cell[e] == 1, "owner cell %zu of (%lld, %lld) written %d times", e, LL(N), LL(G), cell[e]);
    for (size_t e = 0; e < met.size(); ++e) CHECK(met[e] == 1, "stream row %zu of (%lld, %lld) met %d times", e, LL(N), LL(G), met[e]);
}

// The arena of a call: the pieces do not overlap, and every index a kernel forms lands inside the piece it indexes.  The pieces are
// separate arrays of exactly the carved sizes (in 4-byte words; a double is two), so an index out of range is the sanitizer's error;
// a cell that a kernel must write exactly once and is written twice or never is the program's.
struct Pieces {
    std::vector<int32_t> words[g2l::P_COUNT];
    int32_t& f32(int p, int64_t i) { return words[p].data()[i]; }
    int32_t& f64(int p, int64_t i) { words[p].data()[2 * i + 1] += 1; return words[p].data()[2 * i]; }
};

static void once(const Pieces& P, int p, const char* what, int call, int64_t N, int64_t G, int64_t F) {
    for (size_t e = 0; e < P.words[p].size(); ++e)
        CHECK(P.words[p][e] == 1, "%s word %zu of call %d (%lld, %lld, %lld) written %d times", what, e, call, LL(N), LL(G), LL(F), P.words[p][e]);
}

// the padded copy of `rows` rows: k_g2l_pad's writes, then the last word a main kernel reads of the last tile
static void walk_images(Pieces& P, int frag, int rowmajor, bool back, int64_t rows, int64_t F) {
    const int64_t Rp = g2l::padded_rows(rows);
    const int Fp = g2l::padded_features(F);
    for (int64_t e = 0; e < Rp * Fp; ++e) {
        const int64_t i = e / Fp;
        const int k = (int)(e - i * Fp);
        P.f32(frag, infonce::frag_offset(i, k, Fp)) += 1;
        if (back) P.f32(rowmajor, e) += 1;
    }
    const int64_t tile_floats = (int64_t)g2l::TILE * Fp, T = g2l::num_tiles(rows);
    const int nqq = Fp >> 3;
    for (int64_t t = 0; t < T; ++t)
        for (int lane = 0; lane < 64; lane += 63) {   // a lane's 16 bytes of the first and of the last group of a tile
            (void)P.f32(frag, t * tile_floats + (0 * 64 + lane) * 4 + 0);
            (void)P.f32(frag, t * tile_floats + ((nqq - 1) * 64 + lane) * 4 + 3);
            if (back) (void)P.f32(rowmajor, t * tile_floats + tile_floats - 1);
        }
}

static void check_arena(int call, int64_t N, int64_t G, int64_t F) {
    const g2l::Arena A = g2l::arena(call, N, G, F);
    std::vector<unsigned char> mem((size_t)(A.bytes / 4 + 1), 0);
    Pieces P;
    for (int p = 0; p < g2l::P_COUNT; ++p) {
        if (A.off[p] < 0) { CHECK(A.size[p] == 0, "absent piece %d has a size", p); continue; }
        CHECK((A.off[p] & 255) == 0 && (A.size[p] & 3) == 0 && A.off[p] + A.size[p] <= A.bytes, "piece %d of call %d (%lld, %lld, %lld)", p, call, LL(N), LL(G), LL(F));
        for (int64_t w = 0; w < A.size[p] / 4; ++w) {
            unsigned char& m = mem[(size_t)(A.off[p] / 4 + w)];
            CHECK(m == 0, "pieces overlap at byte %lld", LL(A.off[p] + 4 * w));
            m = 1;
        }
        P.words[p].assign((size_t)(A.size[p] / 4), 0);
    }
    const int64_t Np = g2l::padded_rows(N), Gp = g2l::padded_rows(G), parts = g2l::num_parts(N, G, F), nc = spmm::num_chunks(N);
    const int Fp = g2l::padded_features(F), nft = Fp / g2l::TILE;
    const bool jsd = call == g2l::JSD_FORWARD || call == g2l::JSD_BACKWARD, back = call == g2l::JSD_BACKWARD || call == g2l::BOOT_BACKWARD;
    if (jsd && G >= 2) {
        for (int64_t i = 0; i < Np; ++i) P.f32(g2l::P_MAP, i) += 1;                        // k_g2l_map; the main kernels read rows < Np
        once(P, g2l::P_MAP, "map", call, N, G, F);
        walk_images(P, g2l::P_HFRAG, g2l::P_HROWS, back, N, F);
        walk_images(P, g2l::P_GFRAG, g2l::P_GROWS, back, G, F);
        once(P, g2l::P_HFRAG, "node fragment image", call, N, G, F);
        once(P, g2l::P_GFRAG, "graph fragment image", call, N, G, F);
        if (back) {
            once(P, g2l::P_HROWS, "node row image", call, N, G, F);
            once(P, g2l::P_GROWS, "graph row image", call, N, G, F);
            // the dg kernel's stores: block -> (graph row block, part), wave -> owner tile, lane and register -> cell
            const int64_t To = g2l::num_tiles(G), RB = g2l::row_blocks(G);
            for (int64_t block = 0; block < RB * parts; ++block) {
                const int64_t blk = block % RB, part = block / RB;
                for (int wave = 0; wave < g2l::BLOCK_TILES; ++wave) {
                    const int64_t ot = blk * g2l::BLOCK_TILES + wave;
                    if (ot >= To) continue;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int ft = 0; ft < nft; ++ft)
                            for (int r = 0; r < 16; ++r)
                                P.f32(g2l::P_PARTIAL, (part * Gp + ot * g2l::TILE) * Fp + (lane & 31) + (int64_t)g2l::reg_row(r, lane >> 5) * Fp + ft * g2l::TILE) += 1;
                }
            }
            once(P, g2l::P_PARTIAL, "part accumulator", call, N, G, F);
            for (int64_t p = 0; p < parts; ++p) (void)P.f32(g2l::P_PARTIAL, (p * Gp + (G - 1)) * Fp + (F - 1));   // k_g2l_dg_finish
        }
    } else if (jsd && back) {
        for (int pass = 0; pass < 2; ++pass)
            for (int64_t i = 0; i < N; ++i) P.f32(g2l::P_W, pass * N + i) += 1;              // k_g2l_vec
        for (int64_t p = 0; p < parts; ++p)
            for (int64_t k = 0; k < F; ++k) P.f32(g2l::P_PARTIAL, p * F + k) += 1;           // k_g2l_dg_vec
        once(P, g2l::P_W, "weight", call, N, G, F);
        once(P, g2l::P_PARTIAL, "part accumulator", call, N, G, F);
    }
    if (!jsd) {
        for (int64_t i = 0; i < N; ++i) P.f32(g2l::P_MAP, i) += 1;
        for (int64_t j = 0; j < G; ++j)
            for (int64_t k = 0; k < F; ++k) P.f32(g2l::P_GHAT, j * F + k) += 1;
        once(P, g2l::P_MAP, "map", call, N, G, F);
        once(P, g2l::P_GHAT, "hat image", call, N, G, F);
    }
    if (!back) {
        for (int64_t q = 0; q < nc * (jsd ? 2 : 1); ++q) P.f64(g2l::P_CSUM, q) += 1;         // k_g2l_chunks
        once(P, g2l::P_CSUM, "chunk sum", call, N, G, F);
    }
}

static void check_vec(int64_t N, int64_t F) {
    const int R = g2l::vec_rows(F), Fs = g2l::vec_stride(F);
    CHECK(R >= 32 && R <= g2l::VEC_THREADS && (R & (R - 1)) == 0, "rows of a block at F = %lld: %d", LL(F), R);
    CHECK((Fs & 1) == 1 && Fs >= F && Fs <= F + 1, "row stride at F = %lld", LL(F));
    CHECK((int64_t)R * Fs * 4 <= g2l::VEC_LDS_BYTES, "LDS of a block at F = %lld", LL(F));
    std::vector<float> lds((size_t)(R * Fs), 0.0f);
    std::vector<int> seen((size_t)N, 0);
    for (int64_t blk = 0; blk < g2l::vec_blocks(N, F); ++blk) {
        const int64_t i0 = blk * R;
        const int nrows = (int)(N - i0 < R ? N - i0 : R);
        CHECK(nrows >= 1, "an empty block");
        CHECK((i0 * F * 4) % 16 == 0, "a block's first row is not 16-byte aligned");
        // the staging: 16-byte pieces that may cross rows, then the tail
        const int total = nrows * (int)F, nvec = total >> 2;
        for (int q = 0; q < nvec; ++q) {
            int r = (q << 2) / (int)F, k = (q << 2) - r * (int)F;
            for (int u = 0; u < 4; ++u) {
                lds[(size_t)(r * Fs + k)] += 1.0f;
                if (++k == F) { k = 0; ++r; }
            }
        }
        for (int e = nvec << 2; e < total; ++e) lds[(size_t)((e / (int)F) * Fs + e % (int)F)] += 1.0f;
        for (int r = 0; r < nrows; ++r) {
            for (int k = 0; k < F; ++k) { CHECK(lds[(size_t)(r * Fs + k)] == 1.0f, "LDS cell (%d, %d) staged %g times", r, k, lds[(size_t)(r * Fs + k)]); lds[(size_t)(r * Fs + k)] = 0.0f; }
            ++seen[(size_t)(i0 + r)];
        }
    }
    for (int64_t i = 0; i < N; ++i) CHECK(seen[(size_t)i] == 1, "row %lld of %lld in %d blocks", LL(i), LL(N), seen[(size_t)i]);
}

static void check_ng(int64_t N, int64_t G) {
    const int64_t F = 1 + (N * 7 + G) % 100;
    const int64_t T = g2l::num_tiles(N), P = g2l::num_parts(N, G, F);
    CHECK(P >= 1 && P <= T && g2l::part_begin(N, G, F, 0) == 0 && g2l::part_begin(N, G, F, P) == T, "parts of (%lld, %lld): %lld", LL(N), LL(G), LL(P));
    CHECK(g2l::num_neg(N, G) == (G == 1 ? N : N * (G - 1)), "negatives of (%lld, %lld)", LL(N), LL(G));
    check_map(N, G);
    if (G >= 2) {
        check_main(N, G, 1, N, G, F, false);    // forward and dh: the nodes own, the graphs stream whole
        check_main(G, N, P, N, G, F, true);     // dg: the graphs own, the nodes stream in parts
    } else {
        // dg of a single graph: every node in exactly one part
        std::vector<int> seen((size_t)N, 0);
        for (int64_t p = 0; p < P; ++p) {
            const int64_t ib = g2l::part_begin(N, 1, F, p) * g2l::TILE;
            int64_t ie = g2l::part_begin(N, 1, F, p + 1) * g2l::TILE;
            ie = ie < N ? ie : N;
            CHECK(ib < ie, "part %lld of %lld is empty", LL(p), LL(N));
            for (int64_t i = ib; i < ie; ++i) ++seen[(size_t)i];
        }
        for (int64_t i = 0; i < N; ++i) CHECK(seen[(size_t)i] == 1, "node %lld of %lld in %d parts", LL(i), LL(N), seen[(size_t)i]);
    }
    for (int call = 0; call < 4; ++call) check_arena(call, N, G, F);
}

// the rule of launch_backward_main (rlap_infonce.h's, which both backward kernels of the JSD take) and the rows of a block of the
// vector kernels, for every F the exports accept
static void check_instances() {
    int rows_prev = g2l::VEC_THREADS;
    for (int64_t F = 1; F <= g2l::MAX_F; ++F) {
        const int nft = g2l::padded_features(F) / g2l::TILE, inst = infonce::main_instance(nft);
        const bool known = inst == 1 || inst == 2 || inst == 4 || inst == 8 || inst == 16;
        CHECK(known, "instance %d of F = %lld is not one the launchers have", inst, LL(F));
        CHECK(inst >= nft && (inst == 1 || inst / 2 < nft), "instance %d of F = %lld (%d tiles)", inst, LL(F), nft);
        if (known && inst >= nft) {
            std::vector<int> acc((size_t)inst, 0);                       // f32x16 acc[NFT]
            for (int ft = 0; ft < inst; ++ft)
                if (ft < nft) ++acc[(size_t)ft];
            for (int ft = 0; ft < nft; ++ft) CHECK(acc[(size_t)ft] == 1, "tile %d of F = %lld", ft, LL(F));
        }
        const int R = g2l::vec_rows(F);
        CHECK((R == 32 || R == 64 || R == 128 || R == 256) && R <= rows_prev, "rows of a block at F = %lld: %d after %d", LL(F), R, rows_prev);
        CHECK(R == 32 || (int64_t)R * g2l::vec_stride(F) * 4 <= g2l::VEC_LDS_BYTES, "LDS of a block at F = %lld", LL(F));
        CHECK(R == g2l::VEC_THREADS || (int64_t)2 * R * g2l::vec_stride(F) * 4 > g2l::VEC_LDS_BYTES, "a block at F = %lld could hold twice its rows", LL(F));
        rows_prev = R;
    }
    CHECK(g2l::vec_rows(65) == 256 && g2l::vec_rows(66) == 128 && g2l::vec_rows(131) == 128 && g2l::vec_rows(132) == 64 &&
          g2l::vec_rows(263) == 64 && g2l::vec_rows(264) == 32 && g2l::vec_rows(512) == 32, "the edges of vec_rows");
}

int main(int argc, char** argv) {
    const int64_t bound = argc > 1 ? std::atoll(argv[1]) : 300;
    check_reg_rows();
    check_instances();
    for (int64_t F : {65, 66, 131, 132, 263, 264}) check_vec(513, F);   // a last block of one row on either side of every edge
    for (int64_t N = 1; N <= bound; ++N) {
        const int64_t gs[] = {1, 2, 31, 32, 33, 65, N, N + 3};
        for (int64_t G : gs) check_ng(N, G);
    }
    const int64_t fs[] = {1, 2, 3, 4, 5, 31, 32, 33, 100, 255, 256, 511, 512};
    const int64_t ns[] = {1, 31, 32, 33, 65, 257, 300};
    for (int64_t N : ns)
        for (int64_t F : fs) {
            check_vec(N, F);
            for (int call = 0; call < 4; ++call) { check_arena(call, N, 1, F); check_arena(call, N, 33, F); }
        }
    // large sizes: the arithmetic stays in range (no arrays)
    const int64_t big[] = {2708, 169343, 4194304, ((int64_t)1 << 31) - 1};
    for (int64_t N : big)
        for (int64_t G : {(int64_t)1, (int64_t)128, (int64_t)1024, ((int64_t)1 << 31) - 1}) {
            const int64_t P = g2l::num_parts(N, G, 64), T = g2l::num_tiles(N);
            CHECK(P >= 1 && P <= 1024 && g2l::part_begin(N, G, 64, P) == T && g2l::part_begin(N, G, 64, 0) == 0, "parts of (%lld, %lld)", LL(N), LL(G));
            for (int64_t p = 0; p < P; ++p) CHECK(g2l::part_begin(N, G, 64, p) < g2l::part_begin(N, G, 64, p + 1), "part %lld of (%lld, %lld)", LL(p), LL(N), LL(G));
            CHECK(g2l::num_neg(N, G) > 0, "negatives of (%lld, %lld) overflow", LL(N), LL(G));
        }
    std::printf("%lld sizes, %lld failures\n", (long long)bound, (long long)failures);
    return failures ? 1 : 0;
}
