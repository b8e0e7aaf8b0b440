// The index arithmetic of the fused InfoNCE loss (rlap_amd/csrc/rlap_infonce.h) as a stand-alone program, built with
// -fsanitize=address,undefined by tests/test_infonce_cpu.py: for every N up to the bound given on the command line it walks the parts,
// the tiles, the register-to-row map, the workgroup map of the main kernels, the fragment image and the chunk finish (and, for every
// F from 1 to 512, the instance of the backward kernels that the launchers choose) through arrays
// of exactly the sizes the library carves, so that an index out of range is an error of the sanitizer and a cell visited twice or
// never one of the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rlap_infonce.h"

using namespace rlap;

static int64_t failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } ++failures; } } while (0)

static void check_reg_rows() {
    int seen[32];
    std::memset(seen, 0, sizeof seen);
    for (int h = 0; h < 2; ++h)
        for (int r = 0; r < 16; ++r) {
            const int row = infonce::reg_row(r, h);
            CHECK(row >= 0 && row < 32, "reg_row(%d, %d) = %d", r, h, row);
            CHECK(row == infonce::reg_row(r, 0) + 4 * h, "half offset of register %d", r);
            if (row >= 0 && row < 32) ++seen[row];
        }
    for (int i = 0; i < 32; ++i) CHECK(seen[i] == 1, "row %d is held %d times", i, seen[i]);
}

static void check_n(int64_t N) {
    const int64_t T = infonce::num_tiles(N), RB = infonce::row_blocks(N), Np = infonce::padded_rows(N), P = infonce::num_parts(N);
    CHECK(T == (N + 31) / 32 && Np == 32 * T && Np >= N && Np < N + 32, "tiles of %lld", (long long)N);
    CHECK(RB * infonce::BLOCK_TILES >= T && (RB - 1) * infonce::BLOCK_TILES < T, "row blocks of %lld", (long long)N);
    CHECK(P >= 1 && P <= T, "parts of %lld: %lld", (long long)N, (long long)P);
    CHECK(infonce::part_begin(N, 0) == 0 && infonce::part_begin(N, P) == T, "ends of the parts of %lld", (long long)N);
    // every column once, through parts, tiles, registers and halves
    std::vector<int> col((size_t)N, 0);
    for (int64_t p = 0; p < P; ++p) {
        const int64_t tb = infonce::part_begin(N, p), te = infonce::part_begin(N, p + 1);
        CHECK(tb < te, "part %lld of %lld is empty", (long long)p, (long long)N);
        for (int64_t t = tb; t < te; ++t)
            for (int r = 0; r < 16; ++r)
                for (int h = 0; h < 2; ++h) {
                    const int64_t j = t * infonce::TILE + infonce::reg_row(r, h);
                    CHECK(j < Np, "column %lld beyond the padded rows", (long long)j);
                    if (j < N) ++col[(size_t)j];
                }
    }
    for (int64_t j = 0; j < N; ++j) CHECK(col[(size_t)j] == 1, "column %lld of %lld summed %d times", (long long)j, (long long)N, col[(size_t)j]);
    // the workgroup map: block -> (row block, part), wave -> owner tile; every (part, owner row) cell of the part sums written once
    std::vector<int> zpart((size_t)(P * Np), 0), diag((size_t)Np, 0);
    for (int64_t block = 0; block < RB * P; ++block) {
        const int64_t blk = block % RB, part = block / RB;
        for (int wave = 0; wave < infonce::BLOCK_TILES; ++wave) {
            const int64_t ot = blk * infonce::BLOCK_TILES + wave;
            if (ot >= T) continue;
            for (int c = 0; c < 32; ++c) {
                const int64_t orow = ot * infonce::TILE + c;
                ++zpart[(size_t)(part * Np + orow)];
                for (int64_t t = infonce::part_begin(N, part); t < infonce::part_begin(N, part + 1); ++t)
                    for (int r = 0; r < 16; ++r)
                        for (int h = 0; h < 2; ++h)
                            if (t * infonce::TILE + infonce::reg_row(r, h) == orow) ++diag[(size_t)orow];
            }
        }
    }
    for (size_t e = 0; e < zpart.size(); ++e) CHECK(zpart[e] == 1, "part sum cell %zu of %lld written %d times", e, (long long)N, zpart[e]);
    for (int64_t i = 0; i < Np; ++i) CHECK(diag[(size_t)i] == 1, "diagonal of row %lld of %lld met %d times", (long long)i, (long long)N, diag[(size_t)i]);
    // the chunk finish: chunk sums in an array of num_chunks(N), then their sum, against the rule in one piece
    std::vector<double> rows((size_t)N), csum((size_t)spmm::num_chunks(N));
    for (int64_t i = 0; i < N; ++i) rows[(size_t)i] = 1.0 / (double)(3 * i + 1) - 0.25;
    for (int64_t k = 0; k < spmm::num_chunks(N); ++k)
        csum[(size_t)k] = spmm::chunk_sum(N, k, [](int64_t) { return 1.0; }, [&](int64_t e) { return rows[(size_t)e]; });
    double total = 0.0;
    for (int64_t k = 0; k < spmm::num_chunks(N); ++k) total = total + csum[(size_t)k];
    const double whole = spmm::list_sum(N, [](int64_t) { return 1.0; }, [&](int64_t e) { return rows[(size_t)e]; }, false, 0.0, 0.0);
    CHECK(std::memcmp(&total, &whole, 8) == 0, "chunk finish of %lld", (long long)N);
}

// the fragment image is a bijection of the padded (row, column) cells
static void check_frag(int64_t N, int64_t F) {
    const int64_t Np = infonce::padded_rows(N);
    const int Fp = infonce::padded_features(F);
    CHECK(Fp % 32 == 0 && Fp >= F && Fp < F + 32, "padded features of %lld", (long long)F);
    std::vector<int> cell((size_t)(Np * Fp), 0);
    for (int64_t i = 0; i < Np; ++i)
        for (int k = 0; k < Fp; ++k) {
            const int64_t o = infonce::frag_offset(i, k, Fp);
            CHECK(o >= 0 && o < Np * Fp, "fragment offset (%lld, %d) = %lld", (long long)i, k, (long long)o);
            if (o >= 0 && o < Np * Fp) ++cell[(size_t)o];
            // what a lane reads: tile t, group qq of four k-pairs, lane 32 (k & 1) + row, element (k >> 1) & 3
            const int64_t lane_read = (((i >> 5) * (Fp >> 3) + (k >> 3)) * 64 + (k & 1) * 32 + (i & 31)) * 4 + ((k >> 1) & 3);
            CHECK(o == lane_read, "fragment offset (%lld, %d) is not the lane's", (long long)i, k);
        }
    for (size_t e = 0; e < cell.size(); ++e) CHECK(cell[e] == 1, "fragment cell %zu of (%lld, %lld) written %d times", e, (long long)N, (long long)F, cell[e]);
}

// the rule of launch_backward_main for every F the exports accept: an instance the launchers have, the smallest that holds nft; the
// accumulator tiles a wave of that instance indexes (ft < NFT) cover the live ones (ft < nft) and stay inside its array
static void check_instances() {
    int used[17];
    std::memset(used, 0, sizeof used);
    for (int64_t F = 1; F <= infonce::MAX_F; ++F) {
        const int nft = infonce::feature_tiles(F), inst = infonce::main_instance(nft);
        CHECK(nft * infonce::TILE == infonce::padded_features(F) && nft >= 1 && nft <= 16, "feature tiles of %lld", (long long)F);
        const bool known = inst == 1 || inst == 2 || inst == 4 || inst == 8 || inst == 16;
        CHECK(known, "instance %d of F = %lld is not one the launchers have", inst, (long long)F);
        CHECK(inst >= nft, "instance %d of F = %lld holds fewer than %d tiles", inst, (long long)F, nft);
        CHECK(inst == 1 || inst / 2 < nft, "instance %d of F = %lld is not the smallest for %d tiles", inst, (long long)F, nft);
        if (!known || inst < nft) continue;
        std::vector<int> acc((size_t)inst, 0);                           // f32x16 acc[NFT]
        for (int ft = 0; ft < inst; ++ft)
            if (ft < nft) ++acc[(size_t)ft];
        for (int ft = 0; ft < nft; ++ft) CHECK(acc[(size_t)ft] == 1, "tile %d of F = %lld", ft, (long long)F);
        ++used[inst];
    }
    CHECK(used[1] == 32 && used[2] == 32 && used[4] == 64 && used[8] == 128 && used[16] == 256, "the instances' shares of F = 1 .. 512");
    CHECK(infonce::main_instance(0) == 0 && infonce::main_instance(17) == 0 && infonce::main_instance(-1) == 0, "no instance outside 1 .. 16 tiles");
}

int main(int argc, char** argv) {
    const int64_t bound = argc > 1 ? std::atoll(argv[1]) : 300;
    check_reg_rows();
    check_instances();
    for (int64_t N = 1; N <= bound; ++N) check_n(N);
    const int64_t fs[] = {1, 2, 3, 31, 32, 33, 100, 256, 512};
    const int64_t ns[] = {1, 31, 32, 33, 65, 129, 300};
    for (int64_t N : ns)
        for (int64_t F : fs) check_frag(N, F);
    // large N: the arithmetic stays in range (no arrays)
    const int64_t big[] = {2708, 34493, 169343, ((int64_t)1 << 31) - 1};
    for (int64_t N : big) {
        const int64_t P = infonce::num_parts(N), T = infonce::num_tiles(N);
        CHECK(P >= 1 && P <= 256 && infonce::part_begin(N, P) == T && infonce::part_begin(N, 0) == 0, "parts of %lld", (long long)N);
        for (int64_t p = 0; p < P; ++p) CHECK(infonce::part_begin(N, p) < infonce::part_begin(N, p + 1), "part %lld of %lld", (long long)p, (long long)N);
    }
    // tau's range
    CHECK(infonce::tau_ok(1.0 / 32.0) && infonce::tau_ok(1024.0) && infonce::tau_ok(0.4), "tau inside");
    CHECK(!infonce::tau_ok(0.0) && !infonce::tau_ok(0.03) && !infonce::tau_ok(1025.0) && !infonce::tau_ok(-1.0) && !infonce::tau_ok((double)NAN), "tau outside");
    std::printf("%lld sizes, %lld failures\n", (long long)bound, (long long)failures);
    return failures ? 1 : 0;
}
