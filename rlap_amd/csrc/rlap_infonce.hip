// rlap_infonce.hip -- the fused InfoNCE contrastive loss, forward and backward (rlap_infonce / rlap_infonce_backward):
// DualBranchContrast(InfoNCEBatched(tau), mode="L2L") of the node-level training step without the N x N similarity matrix.  The
// similarities come from v_mfma_f32_32x32x2_f32 -- bit for bit a k-ordered float32 fmaf chain --, live in registers and are never
// written to memory; every sum has the fixed order of rlap_infonce.h; the backward pass recomputes the similarities with the same
// chain.  Memory is O(N F).  A translation unit of its own.
//
//   pre-pass   the float64 squared norms (one thread per row, sequential as the rule says), then the normalised copies ah, bh in the
//              arena, zero-padded to 32-row tiles and to a multiple of 32 columns, in two images: row-major, and the FRAGMENT image
//              (infonce::frag_offset) in which the 16 bytes of a lane are its operands of four consecutive MFMAs, so that a tile is
//              one contiguous block that waves read 1 KiB an instruction.
//   main       one template for the three kernels.  A workgroup of four waves OWNS four 32-row tiles (one per wave) of one input
//              and walks the 32-row tiles of the other input, the STREAM, over its part of them (infonce::num_parts: small N is
//              split so that the chip fills); a stream tile's fragment image (backward: and its row-major image) is staged through
//              LDS once for the four waves: 32 KB (64 KB) at F = 256, 64 KB (128 KB) at F = 512.
//              Per tile a wave computes X[stream row][owner row] = the chain over F -- stream as the A operand, owner as B, so the
//              owner is on the lane and the stream rows are in the 16 registers (infonce::reg_row).
//                forward   e = expw((X - 1) / tau) added in register order into the lane's float64 sum; the diagonal is kept.
//                backward  p = e * (1 / Z_anchor); the accumulator tile is then the A operand of the next MFMAs as it stands
//                          (register r of the two lane halves holds stream rows reg_row(r, 0), reg_row(r, 1): the k pair of
//                          step r), the B operand being the stream's row-major image in LDS: D[owner row][32 columns] per feature tile,
//                          F / 32 accumulator tiles per wave (256 registers at F = 512, the AGPR half included).
//              anchor-owner and sample-owner backward kernels are the same code with the inputs swapped; 1 / Z belongs to the
//              anchor, which is the lane in one and the register's row in the other.
//   finish     forward: Z = the part sums in order, the row terms, the chunk-rule sum of them, the loss.  backward: the part
//              accumulators added in order, then the float64 push through the normalisation, one wave per row.
// No float atomics, no host synchronisation, nothing allocated outside the arena.  Every address is formed from the padded sizes:
// a wave whose owner tile lies behind the last one only takes part in the staging.
//
// The symmetric pair (rlap_infonce_pair / rlap_infonce_pair_backward) computes 0.5 * (l(a, b) + l(b, a)) from one pass:
// its forward main kernel k_in_pair_main takes the row sums Z and the column sums Zc from the same tiles, its backward is k_in_main
// with the weight e (1 / Z_i + 1 / Zc_j) (IN_BACK_PAIR), its finish the one above for two lists.
//
// Intraview negatives (rlap_infonce_intra and its three kin) are further instances of k_in_main: IN_FWD_INTRA, a forward
// pass whose owner and stream are the same view, with the diagonal left out or kept, whose part sums follow the row sum's in the
// float64 chain of Z; IN_BACK_ANCHOR_INTRA and IN_BACK_PAIR_INTRA, which walk a part's tiles of the other view and then the same tiles
// of the owner's own view into ONE accumulator, the second with the weight e (1 / Z_i + 1 / Z_j).  The instances above are unchanged.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/rlap_hip.h"
#include "rlap_infonce.h"
#include "rlap_infonce_api.h"
#include "rlap_spmm.h"
#include "rlap_tile32_dev.h"

namespace rlap {
namespace {

using tile32::f32x16;

constexpr int IN_THREADS = 256;                 // four waves: infonce::BLOCK_TILES owner tiles
constexpr int64_t IN_MAX_GRID = 1 << 20;        // workgroups of an elementwise launch (the kernels stride)
static_assert(IN_THREADS == 64 * infonce::BLOCK_TILES, "one wave per owner tile");

inline unsigned in_blocks(int64_t n, int per_block) { return capped_blocks(n, per_block, IN_MAX_GRID); }

// ------------------------------------------------------------------------------------------------ pre-pass
__global__ __launch_bounds__(256) void k_in_norms(const float* __restrict__ a, const float* __restrict__ b, int64_t N, int64_t F,
                                                  double* __restrict__ n2a, double* __restrict__ n2b) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < 2 * N; t += (int64_t)gridDim.x * blockDim.x) {
        const bool second = t >= N;
        const int64_t i = second ? t - N : t;
        (second ? n2b : n2a)[i] = infonce::norm2((second ? b : a) + i * F, F);
    }
}

// the normalised copy of x, padded with zeros: the fragment image and (rows != nullptr) the row-major image
__global__ __launch_bounds__(256) void k_in_hats(const float* __restrict__ x, const double* __restrict__ n2, int64_t N, int64_t F,
                                                 int64_t Np, int Fp, float* __restrict__ frag, float* __restrict__ rows) {
    const int64_t elems = Np * Fp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < elems; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / Fp;
        const int k = (int)(e - i * Fp);
        float v = 0.0f;
        if (i < N && k < F) v = infonce::hat(x[i * F + k], infonce::norm_of(n2[i]));
        frag[infonce::frag_offset(i, k, Fp)] = v;
        if (rows) rows[e] = v;
    }
}

__global__ __launch_bounds__(256) void k_in_recip(const double* __restrict__ z, int64_t N, int64_t Np, float* __restrict__ rz) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < Np; i += (int64_t)gridDim.x * blockDim.x)
        rz[i] = i < N ? infonce::recip_z(z[i]) : 0.0f;
}

// ------------------------------------------------------------------------------------------------ main
struct Main {
    const float* own_frag; const float* str_frag;   // fragment images, Np x Fp each
    const float* str_rows;                          // backward: the stream's row-major image
    const float* rz;                                // backward: [Np] 1 / Z of the anchors, 0 behind N (pair: of the owner's rows)
    const float* rz2;                               // pair backward: [Np] the reciprocals of the stream's rows, 0 behind N
    float itf;                                      // (float)(1 / tau)
    int64_t N, Np, T, RB; int parts; int Fp; int nft;
    double* zpart; float* sdiag;                    // forward: [parts, Np] part sums of Z; [Np] the diagonal
    float* partial;                                 // backward: [parts, Np, Fp] part accumulators
    const float* own_rows;                          // intraview backward: the owner's row-major image, the second stream's
    int mask_diag;                                  // intraview: 1 leaves the owner's own row out of the intraview stream (INTRA_MASKED)
};

// IN_BACK_PAIR: the weight of the symmetric pair, w = e * (rz[owner row] + rz2[stream row]), for either owner.
// The intraview instances: IN_FWD_INTRA is the forward pass whose stream is the owner's own view -- it leaves the
// diagonal of S alone and, masked, leaves e_ii out; IN_BACK_ANCHOR_INTRA and IN_BACK_PAIR_INTRA walk the part's tiles twice into the
// one accumulator: the other view with the weight of IN_BACK_ANCHOR / IN_BACK_PAIR, then the owner's own view with
// w = e * (rz[owner row] + rz[stream row]), the masked diagonal entering as a zero weight.
enum { IN_FORWARD = 0, IN_BACK_ANCHOR = 1, IN_BACK_SAMPLE = 2, IN_BACK_PAIR = 3, IN_FWD_INTRA = 4, IN_BACK_ANCHOR_INTRA = 5, IN_BACK_PAIR_INTRA = 6 };
constexpr bool in_forward(int mode) { return mode == IN_FORWARD || mode == IN_FWD_INTRA; }
constexpr bool in_intra(int mode) { return mode >= IN_FWD_INTRA; }
constexpr bool in_lane_rz(int mode) { return mode != IN_BACK_SAMPLE && !in_forward(mode); }

template <int NFT, int MODE>
__global__ __launch_bounds__(IN_THREADS) void k_in_main(Main a) {
    extern __shared__ __attribute__((aligned(16))) float in_lds[];   // 32 x Fp floats: the stream tile's fragment image; backward: and its row-major image
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    const int64_t blk = (int64_t)blockIdx.x % a.RB, part = (int64_t)blockIdx.x / a.RB;
    const int64_t ot = blk * infonce::BLOCK_TILES + wave;
    const bool active = ot < a.T;                                    // (wave-uniform)
    const int64_t tile_floats = (int64_t)infonce::TILE * a.Fp;
    const int tile_vec = (int)(tile_floats >> 2), nqq = a.Fp >> 3;
    const float4* __restrict__ owner = reinterpret_cast<const float4*>(a.own_frag + (active ? ot : 0) * tile_floats);
    const int64_t orow = ot * infonce::TILE + c;                     // the lane's owner row (< Np when active)
    const int64_t tb = infonce::part_begin(a.N, part), te = infonce::part_begin(a.N, part + 1);

    double zsum = 0.0;
    float rz_lane = 0.0f;
    if (in_lane_rz(MODE) && active) rz_lane = a.rz[orow];
    f32x16 acc[NFT];
    if (!in_forward(MODE)) tile32::zero_tiles(acc);

    if (!in_intra(MODE)) {
#pragma unroll 1
        for (int64_t t = tb; t < te; ++t) {
            __syncthreads();   // (the previous tile has been read)
            tile32::stage_tile<IN_THREADS>(in_lds, a.str_frag + t * tile_floats, MODE != IN_FORWARD ? a.str_rows + t * tile_floats : nullptr, tile_vec);
            __syncthreads();
            if (!active) continue;
            f32x16 x = tile32::pair_chain(reinterpret_cast<const float4*>(in_lds), owner, nqq, lane);
            const int64_t srow0 = t * infonce::TILE;
            if (MODE == IN_FORWARD) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t srow = srow0 + infonce::reg_row(r, h);
                    const float e = infonce::expw(infonce::exp_arg(x[r], a.itf));
                    const double z2 = zsum + (double)e;
                    zsum = srow < a.N ? z2 : zsum;
                    if (srow == orow) a.sdiag[orow] = x[r];   // (once per owner row of the call: the tile t == ot of one part)
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t srow = srow0 + infonce::reg_row(r, h);
                    const float e = infonce::expw(infonce::exp_arg(x[r], a.itf));
                    float p;
                    if (MODE == IN_BACK_PAIR) {
                        p = infonce::pair_weight(e, rz_lane, a.rz2[srow]);
                    } else {
                        const float rz = MODE == IN_BACK_ANCHOR ? rz_lane : a.rz[srow];   // (srow < Np; 0 behind N)
                        p = infonce::prob(e, rz);
                    }
                    x[r] = srow < a.N ? p : 0.0f;
                }
                tile32::accumulate_tiles(acc, a.nft, x, in_lds + (int)tile_floats, a.Fp, c, h);
            }
        }
    } else {
        // the intraview instances: the same steps; the backward ones walk the part's tiles of the other view, then the same tiles of
        // the owner's own view (`intra`), into the one accumulator
#pragma unroll 1
        for (int pass = 0; pass < (in_forward(MODE) ? 1 : 2); ++pass) {
            const bool intra = in_forward(MODE) || pass == 1;            // (uniform) the stream is the owner's own view
            const float* __restrict__ sfrag = intra ? a.own_frag : a.str_frag;
            const float* __restrict__ srows = intra ? a.own_rows : a.str_rows;
            const float* __restrict__ rzs = intra ? a.rz : a.rz2;        // the reciprocals of the stream's rows (the owner's list in its own view)
            const int64_t skip = intra && a.mask_diag ? orow : -1;       // the stream row that is left out
#pragma unroll 1
            for (int64_t t = tb; t < te; ++t) {
                __syncthreads();   // (the previous tile has been read)
                tile32::stage_tile<IN_THREADS>(in_lds, sfrag + t * tile_floats, !in_forward(MODE) ? srows + t * tile_floats : nullptr, tile_vec);
                __syncthreads();
                if (!active) continue;
                f32x16 x = tile32::pair_chain(reinterpret_cast<const float4*>(in_lds), owner, nqq, lane);
                const int64_t srow0 = t * infonce::TILE;
                if (in_forward(MODE)) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t srow = srow0 + infonce::reg_row(r, h);
                        const float e = infonce::expw(infonce::exp_arg(x[r], a.itf));
                        const double z2 = zsum + (double)e;
                        zsum = srow < a.N && srow != skip ? z2 : zsum;   // (the diagonal of S^ab is the other pass's to keep)
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t srow = srow0 + infonce::reg_row(r, h);
                        const float e = infonce::expw(infonce::exp_arg(x[r], a.itf));
                        float p;
                        if (MODE == IN_BACK_PAIR_INTRA || intra) p = infonce::pair_weight(e, rz_lane, rzs[srow]);   // (srow < Np; 0 behind N)
                        else p = infonce::prob(e, rz_lane);
                        x[r] = srow < a.N && srow != skip ? p : 0.0f;
                    }
                    tile32::accumulate_tiles(acc, a.nft, x, in_lds + (int)tile_floats, a.Fp, c, h);
                }
            }
        }
    }

    if (!active) return;
    if (in_forward(MODE)) {
        const double other = __shfl_xor(zsum, 32);
        if (h == 0) a.zpart[part * a.Np + orow] = zsum + other;      // half 0 + half 1
    } else {
        tile32::store_tiles(acc, a.nft, a.partial + (part * a.Np + ot * infonce::TILE) * a.Fp, a.Fp, c, h);
    }
}

// ------------------------------------------------------------------------------------------------ main, the pair's forward
// Both directions from one pass over S.  A workgroup owns one (group of row blocks, part of the stream tiles): the
// owner block outside, the stream tiles inside, staged through LDS per step as in k_in_main.  The row sums stay in registers across
// the inner loop; the column sums of a step are reduced across the 32 owner lanes by the butterfly, handed over by the four waves
// through LDS and added, waves in order, to an LDS array of one double per column of the span, which is flushed to
// colpart[group][column] when the group's blocks are through.  Every barrier is reached by all four waves: a wave whose owner tile
// lies behind the last one stages, hands over zeros and waits with the others.
struct PairMain {
    const float* own_frag; const float* str_frag;   // fragment images of a (owner) and b (stream), Np x Fp each
    float itf;
    int64_t N, Np, T; int groups; int Fp; int span;  // span: infonce::pair_span_tiles(N), what the column array holds
    double* zpart; double* colpart; float* sdiag;   // [parts, Np] part sums of Z; [groups, Np] group sums of Zc; [Np] the diagonal
};

__global__ __launch_bounds__(IN_THREADS) void k_in_pair_main(PairMain a) {
    extern __shared__ __attribute__((aligned(16))) float in_lds[];   // the stream tile's fragment image | col [32 span] | wave sums [4][32]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    const int64_t group = (int64_t)blockIdx.x % a.groups, part = (int64_t)blockIdx.x / a.groups;
    const int64_t tile_floats = (int64_t)infonce::TILE * a.Fp;
    const int tile_vec = (int)(tile_floats >> 2), nqq = a.Fp >> 3;
    double* col = reinterpret_cast<double*>(in_lds + tile_floats);
    double* wsum = col + (int64_t)infonce::TILE * a.span;
    const int64_t bb = infonce::pair_group_begin(a.N, group), be = infonce::pair_group_begin(a.N, group + 1);
    const int64_t tb = infonce::pair_part_begin(a.N, part), te = infonce::pair_part_begin(a.N, part + 1);

#pragma unroll 1
    for (int64_t sb = tb; sb < te; sb += infonce::PAIR_SPAN_TILES) {
        const int64_t se = sb + infonce::PAIR_SPAN_TILES < te ? sb + infonce::PAIR_SPAN_TILES : te;
        const int span_cols = (int)(se - sb) * infonce::TILE;        // (<= 32 span)
        for (int v = threadIdx.x; v < span_cols; v += IN_THREADS) col[v] = 0.0;   // (seen behind the first barrier below: bb < be, sb < se)
#pragma unroll 1
        for (int64_t blk = bb; blk < be; ++blk) {
            const int64_t ot = blk * infonce::BLOCK_TILES + wave;
            const bool active = ot < a.T;                            // (wave-uniform)
            const float4* __restrict__ owner = reinterpret_cast<const float4*>(a.own_frag + (active ? ot : 0) * tile_floats);
            const int64_t orow = ot * infonce::TILE + c;             // the lane's owner row (< Np when active)
            const bool own_live = active && orow < a.N;
            double zsum = 0.0;
#pragma unroll 1
            for (int64_t t = sb; t < se; ++t) {
                __syncthreads();   // (the previous tile and the previous wave sums have been read)
                tile32::stage_tile<IN_THREADS>(in_lds, a.str_frag + t * tile_floats, nullptr, tile_vec);
                __syncthreads();
                if (active) {
                    const f32x16 x = tile32::pair_chain(reinterpret_cast<const float4*>(in_lds), owner, nqq, lane);
                    const int64_t srow0 = t * infonce::TILE;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int64_t srow = srow0 + infonce::reg_row(r, h);
                        const float e = infonce::expw(infonce::exp_arg(x[r], a.itf));
                        const double z2 = zsum + (double)e;
                        zsum = srow < a.N ? z2 : zsum;
                        if (srow == orow) a.sdiag[orow] = x[r];      // (once per owner row of the call)
                        double v = own_live ? (double)e : 0.0;       // tree32 over the 32 owner lanes of the half
                        v = v + __shfl_xor(v, 1);
                        v = v + __shfl_xor(v, 2);
                        v = v + __shfl_xor(v, 4);
                        v = v + __shfl_xor(v, 8);
                        v = v + __shfl_xor(v, 16);
                        if (c == 0) wsum[wave * infonce::TILE + infonce::reg_row(r, h)] = v;
                    }
                } else if (lane < infonce::TILE) {
                    wsum[wave * infonce::TILE + lane] = 0.0;
                }
                __syncthreads();
                if (threadIdx.x < infonce::TILE) {                   // the four waves in order
                    const int j = (int)(t - sb) * infonce::TILE + threadIdx.x;
                    double s = col[j];
#pragma unroll
                    for (int w = 0; w < infonce::BLOCK_TILES; ++w) s = s + wsum[w * infonce::TILE + threadIdx.x];
                    col[j] = s;
                }
            }
            if (active) {
                const double other = __shfl_xor(zsum, 32);
                if (h == 0) {                                        // the slot is this workgroup's alone: no atomic
                    const int64_t slot = part * a.Np + orow;
                    const double before = sb > tb ? a.zpart[slot] : 0.0;
                    a.zpart[slot] = before + (zsum + other);         // 0 + span 0 + span 1 + ...; a span is half 0 + half 1
                }
            }
        }
        __syncthreads();   // (the last step's column sums are in)
        for (int v = threadIdx.x; v < span_cols; v += IN_THREADS) a.colpart[group * a.Np + sb * infonce::TILE + v] = col[v];
        __syncthreads();   // (flushed before the next span clears the array)
    }
}

// ------------------------------------------------------------------------------------------------ finish, forward
__global__ __launch_bounds__(256) void k_in_rows(const double* __restrict__ zpart, const float* __restrict__ sdiag, int64_t N, int64_t Np,
                                                 int parts, double c, double itau, double* __restrict__ z, double* __restrict__ rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        double Z = 0.0;
        for (int p = 0; p < parts; ++p) Z = Z + zpart[p * Np + i];
        z[i] = Z;
        rows[i] = infonce::row_term(c, sdiag[i], itau, Z);
    }
}

__global__ __launch_bounds__(256) void k_in_chunks(const double* __restrict__ rows, int64_t N, double* __restrict__ csum) {
    tile32::chunk_sums(rows, N, 1, csum);
}

// the pair's finish: Z = the parts in order, Zc = the groups in order, the two lists of row terms; z and rows are [2, N]
__global__ __launch_bounds__(256) void k_in_pair_rows(const double* __restrict__ zpart, const double* __restrict__ colpart, const float* __restrict__ sdiag,
                                                      int64_t N, int64_t Np, int parts, int groups, double c, double itau, double* __restrict__ z,
                                                      double* __restrict__ rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        double Z = 0.0, Zc = 0.0;
        for (int p = 0; p < parts; ++p) Z = Z + zpart[p * Np + i];
        for (int q = 0; q < groups; ++q) Zc = Zc + colpart[q * Np + i];
        z[i] = Z;
        z[N + i] = Zc;
        rows[i] = infonce::row_term(c, sdiag[i], itau, Z);
        rows[N + i] = infonce::row_term(c, sdiag[i], itau, Zc);
    }
}

// the same with intraview negatives: the parts of the two intraview sums (zintra: [2, iparts, Np], view a then view b) follow the
// pair's parts and groups in the two float64 chains
__global__ __launch_bounds__(256) void k_in_pair_rows_intra(const double* __restrict__ zpart, const double* __restrict__ colpart,
                                                            const double* __restrict__ zintra, const float* __restrict__ sdiag, int64_t N, int64_t Np,
                                                            int parts, int groups, int iparts, double c, double itau, double* __restrict__ z,
                                                            double* __restrict__ rows) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
        double Z = 0.0, Zc = 0.0;
        for (int p = 0; p < parts; ++p) Z = Z + zpart[p * Np + i];
        for (int p = 0; p < iparts; ++p) Z = Z + zintra[p * Np + i];
        for (int q = 0; q < groups; ++q) Zc = Zc + colpart[q * Np + i];
        for (int p = 0; p < iparts; ++p) Zc = Zc + zintra[(iparts + p) * Np + i];
        z[i] = Z;
        z[N + i] = Zc;
        rows[i] = infonce::row_term(c, sdiag[i], itau, Z);
        rows[N + i] = infonce::row_term(c, sdiag[i], itau, Zc);
    }
}

__global__ __launch_bounds__(256) void k_in_pair_chunks(const double* __restrict__ rows, int64_t N, double* __restrict__ csum) {
    tile32::chunk_sums(rows, N, 2, csum);
}

__global__ void k_in_pair_loss(const double* __restrict__ csum, int64_t N, double* __restrict__ loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t nc = spmm::num_chunks(N);
    double ta = 0.0, tb = 0.0;
    for (int64_t k = 0; k < nc; ++k) ta = ta + csum[k];
    for (int64_t k = 0; k < nc; ++k) tb = tb + csum[nc + k];
    *loss = infonce::pair_loss_of(ta, tb, N);
}

__global__ void k_in_loss(const double* __restrict__ csum, int64_t N, double* __restrict__ loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double total = 0.0;
    for (int64_t k = 0; k < spmm::num_chunks(N); ++k) total = total + csum[k];
    *loss = infonce::loss_of(total, N);
}

// ------------------------------------------------------------------------------------------------ finish, backward
// one wave per owner row, lanes along the columns: the part accumulators are added once, in part order, and the gradient of the
// normalised row is kept in LDS; every lane then takes the dot product over it in column order (the same chain on every lane, the
// LDS reads broadcast), and the lanes push their columns through the normalisation in float64
constexpr int IN_GRAD_WAVES = 4;
__global__ __launch_bounds__(64 * IN_GRAD_WAVES) void k_in_grad(const float* __restrict__ partial, int parts, int64_t N, int64_t F, int64_t Np, int Fp,
                                                                const float* __restrict__ own_rows, const float* __restrict__ other_rows,
                                                                const double* __restrict__ n2, const double* __restrict__ g, double c, double itau,
                                                                int pair, float* __restrict__ out) {
    __shared__ double gh[IN_GRAD_WAVES][infonce::MAX_F];
    __shared__ float oh[IN_GRAD_WAVES][infonce::MAX_F];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double gs = pair ? infonce::pair_grad_scale(*g, N) : infonce::grad_scale(*g, N);   // (pair: c is 2 c)
    for (int64_t base = (int64_t)blockIdx.x * IN_GRAD_WAVES; base < N; base += (int64_t)gridDim.x * IN_GRAD_WAVES) {   // (the same turns for every wave)
        const int64_t i = base + wave;
        const bool live = i < N;
        if (live) {
            for (int k = lane; k < F; k += 64) {
                float D = 0.0f;
                for (int p = 0; p < parts; ++p) D = D + partial[(p * Np + i) * Fp + k];
                gh[wave][k] = infonce::grad_hat(gs, c, other_rows[i * Fp + k], itau, D);
                oh[wave][k] = own_rows[i * Fp + k];
            }
        }
        __syncthreads();
        if (live) {
            const bool clamped = infonce::norm_clamped(n2[i]);
            const double nrm = infonce::norm_of(n2[i]);
            double dot = 0.0;
            for (int k = 0; k < F; ++k) dot = infonce::dot_step(dot, oh[wave][k], gh[wave][k]);
            for (int k = lane; k < F; k += 64) out[i * F + k] = infonce::grad_in(gh[wave][k], oh[wave][k], dot, nrm, clamped);
        }
        __syncthreads();   // (the row has been read before the next one is written)
    }
}

// ------------------------------------------------------------------------------------------------ host
struct Bufs {
    double *n2a, *n2b;
    float *a_frag, *b_frag, *a_rows, *b_rows;
    double* zpart; float* sdiag; double* csum;
    float* rz; float *part_a, *part_b;
    double* colpart; float* rz2;                    // the pair's: the group sums of Zc; the second reciprocal vector
    double* zintra;                                 // the pair's with intraview negatives: [2, num_parts, Np] part sums of the intraview sums
};

// the pair's arena: the one-direction call's with the pair's partial sums (forward) or the second reciprocal vector (backward)
// (intraview negatives: the forward call keeps the part sums of the two intraview sums; the backward call needs nothing more)
size_t carve_pair(Carve& C, int64_t N, int64_t F, bool backward, int intraview, Bufs& B) {
    const int64_t Np = infonce::padded_rows(N), Fp = infonce::padded_features(F);
    B = Bufs{};
    B.n2a = C.take<double>(Np);
    B.n2b = C.take<double>(Np);
    B.a_frag = C.take<float>(Np * Fp);
    B.b_frag = C.take<float>(Np * Fp);
    if (!backward) {
        B.zpart = C.take<double>(infonce::pair_parts(N) * Np);
        B.colpart = C.take<double>(infonce::pair_groups(N) * Np);
        B.sdiag = C.take<float>(Np);
        B.csum = C.take<double>(2 * spmm::num_chunks(N));
        if (intraview != infonce::INTRA_NONE) B.zintra = C.take<double>(2 * infonce::num_parts(N) * Np);
    } else {
        const int64_t parts = infonce::num_parts(N);
        B.a_rows = C.take<float>(Np * Fp);
        B.b_rows = C.take<float>(Np * Fp);
        B.rz = C.take<float>(Np);
        B.rz2 = C.take<float>(Np);
        B.part_a = C.take<float>(parts * Np * Fp);
        B.part_b = C.take<float>(parts * Np * Fp);
    }
    return C.off + 256;
}

// (intraview negatives: the forward call's part sums are the row sum's, then the intraview sum's; the backward call's arena is unchanged)
size_t carve_infonce(Carve& C, int64_t N, int64_t F, bool backward, int intraview, Bufs& B) {
    const int64_t Np = infonce::padded_rows(N), Fp = infonce::padded_features(F), parts = infonce::num_parts(N);
    B = Bufs{};
    B.n2a = C.take<double>(Np);
    B.n2b = C.take<double>(Np);
    B.a_frag = C.take<float>(Np * Fp);
    B.b_frag = C.take<float>(Np * Fp);
    if (!backward) {
        B.zpart = C.take<double>((intraview != infonce::INTRA_NONE ? infonce::intra_z_parts(N) : parts) * Np);
        B.sdiag = C.take<float>(Np);
        B.csum = C.take<double>(spmm::num_chunks(N));
    } else {
        B.a_rows = C.take<float>(Np * Fp);
        B.b_rows = C.take<float>(Np * Fp);
        B.rz = C.take<float>(Np);
        B.part_a = C.take<float>(parts * Np * Fp);
        B.part_b = C.take<float>(parts * Np * Fp);
    }
    return C.off + 256;
}

Main main_args(const InfonceArgs& g) {
    Main m{};
    m.itf = infonce::inv_tau_f(g.tau);
    m.N = g.N; m.Np = infonce::padded_rows(g.N); m.T = infonce::num_tiles(g.N); m.RB = infonce::row_blocks(g.N);
    m.parts = (int)infonce::num_parts(g.N);
    m.Fp = infonce::padded_features(g.F); m.nft = m.Fp / infonce::TILE;
    return m;
}

template <int NFT, int MODE>
int launch_main_t(hipStream_t st, const Main& m) {
    const size_t lds = (size_t)infonce::TILE * m.Fp * sizeof(float) * (in_forward(MODE) ? 1 : 2);
    if (const int rc = tile32::allow_lds(&k_in_main<NFT, MODE>, lds)) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_in_main<NFT, MODE>), dim3((unsigned)(m.RB * m.parts)), dim3(IN_THREADS), lds, st, m);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

template <int MODE>
int launch_backward_main(hipStream_t st, const Main& m) {
    return tile32::ladder_launch(m.nft, [&](auto nft) { return launch_main_t<decltype(nft)::value, MODE>(st, m); });
}

// the forward pass of one view against itself: the part sums of its intraview sum into zpart [num_parts, Np]
int launch_forward_intra(hipStream_t st, Main m, int intraview, const float* frag, double* zpart) {
    m.own_frag = frag; m.str_frag = frag; m.zpart = zpart; m.sdiag = nullptr;
    m.mask_diag = intraview == infonce::INTRA_MASKED;
    return launch_main_t<1, IN_FWD_INTRA>(st, m);
}

int prepass(hipStream_t st, const InfonceArgs& g, const Bufs& B) {
    const int64_t Np = infonce::padded_rows(g.N);
    const int Fp = infonce::padded_features(g.F);
    hipLaunchKernelGGL(k_in_norms, dim3(in_blocks(2 * g.N, 256)), dim3(256), 0, st, g.a, g.b, g.N, g.F, B.n2a, B.n2b);
    hipLaunchKernelGGL(k_in_hats, dim3(in_blocks(Np * Fp, 256)), dim3(256), 0, st, g.a, (const double*)B.n2a, g.N, g.F, Np, Fp, B.a_frag, B.a_rows);
    hipLaunchKernelGGL(k_in_hats, dim3(in_blocks(Np * Fp, 256)), dim3(256), 0, st, g.b, (const double*)B.n2b, g.N, g.F, Np, Fp, B.b_frag, B.b_rows);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace

size_t infonce_bytes(int64_t N, int64_t F, int intraview) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_infonce(C, N, F, false, intraview, B);
}

size_t infonce_backward_bytes(int64_t N, int64_t F, int intraview) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_infonce(C, N, F, true, intraview, B);
}

int infonce_run(hipStream_t st, void* ws, size_t ws_bytes, const InfonceArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_infonce(C, g.N, g.F, false, g.intraview, B) > ws_bytes) return RLAP_E_WORKSPACE;
    if (const int rc = prepass(st, g, B)) return rc;
    Main m = main_args(g);
    m.own_frag = B.a_frag; m.str_frag = B.b_frag; m.zpart = B.zpart; m.sdiag = B.sdiag;
    if (const int rc = launch_main_t<1, IN_FORWARD>(st, m)) return rc;
    int zparts = m.parts;
    if (g.intraview != infonce::INTRA_NONE) {   // the anchors against themselves: the part sums behind the row sum's
        if (const int rc = launch_forward_intra(st, m, g.intraview, B.a_frag, B.zpart + (int64_t)m.parts * m.Np)) return rc;
        zparts = (int)infonce::intra_z_parts(g.N);
    }
    const double c = infonce::positive_coef((g.flags & RLAP_INFONCE_POSITIVE_RAW) != 0, g.tau), itau = infonce::inv_tau(g.tau);
    hipLaunchKernelGGL(k_in_rows, dim3(in_blocks(g.N, 256)), dim3(256), 0, st, (const double*)B.zpart, (const float*)B.sdiag, g.N, m.Np, zparts,
                       c, itau, g.z, g.rows);
    hipLaunchKernelGGL(k_in_chunks, dim3(in_blocks(spmm::num_chunks(g.N), 256)), dim3(256), 0, st, (const double*)g.rows, g.N, B.csum);
    hipLaunchKernelGGL(k_in_loss, dim3(1), dim3(64), 0, st, (const double*)B.csum, g.N, g.loss);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int infonce_backward_run(hipStream_t st, void* ws, size_t ws_bytes, const InfonceArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_infonce(C, g.N, g.F, true, g.intraview, B) > ws_bytes) return RLAP_E_WORKSPACE;
    if (const int rc = prepass(st, g, B)) return rc;
    Main m = main_args(g);
    hipLaunchKernelGGL(k_in_recip, dim3(in_blocks(m.Np, 256)), dim3(256), 0, st, g.z_in, g.N, m.Np, B.rz);
    RLAP_HIPCHK(hipGetLastError());
    m.rz = B.rz;
    const double c = infonce::positive_coef((g.flags & RLAP_INFONCE_POSITIVE_RAW) != 0, g.tau), itau = infonce::inv_tau(g.tau);
    // the anchors own, the samples stream: D = sum_j p_ij bh_j
    m.own_frag = B.a_frag; m.str_frag = B.b_frag; m.str_rows = B.b_rows; m.partial = B.part_a;
    if (g.intraview != infonce::INTRA_NONE) {   // then the anchors themselves, into the same accumulator
        m.own_rows = B.a_rows; m.mask_diag = g.intraview == infonce::INTRA_MASKED;
        if (const int rc = launch_backward_main<IN_BACK_ANCHOR_INTRA>(st, m)) return rc;
    } else if (const int rc = launch_backward_main<IN_BACK_ANCHOR>(st, m)) {
        return rc;
    }
    // the samples own, the anchors stream: D' = sum_i p_ij ah_i
    m.own_frag = B.b_frag; m.str_frag = B.a_frag; m.str_rows = B.a_rows; m.partial = B.part_b;
    if (const int rc = launch_backward_main<IN_BACK_SAMPLE>(st, m)) return rc;
    hipLaunchKernelGGL(k_in_grad, dim3(in_blocks(g.N, IN_GRAD_WAVES)), dim3(64 * IN_GRAD_WAVES), 0, st, (const float*)B.part_a, m.parts, g.N, g.F, m.Np, m.Fp,
                       (const float*)B.a_rows, (const float*)B.b_rows, (const double*)B.n2a, g.g, c, itau, 0, g.ga);
    hipLaunchKernelGGL(k_in_grad, dim3(in_blocks(g.N, IN_GRAD_WAVES)), dim3(64 * IN_GRAD_WAVES), 0, st, (const float*)B.part_b, m.parts, g.N, g.F, m.Np, m.Fp,
                       (const float*)B.b_rows, (const float*)B.a_rows, (const double*)B.n2b, g.g, c, itau, 0, g.gb);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// ------------------------------------------------------------------------------------------------ the symmetric pair
size_t infonce_pair_bytes(int64_t N, int64_t F, int intraview) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_pair(C, N, F, false, intraview, B);
}

size_t infonce_pair_backward_bytes(int64_t N, int64_t F, int intraview) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_pair(C, N, F, true, intraview, B);
}

// LDS of k_in_pair_main: the stream tile's fragment image, the span's column sums, the four waves' sums
size_t infonce_pair_lds_bytes(int64_t N, int64_t F) {
    return (size_t)infonce::TILE * infonce::padded_features(F) * sizeof(float) +
           (size_t)infonce::TILE * (infonce::pair_span_tiles(N) + infonce::BLOCK_TILES) * sizeof(double);
}

int infonce_pair_run(hipStream_t st, void* ws, size_t ws_bytes, const InfonceArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_pair(C, g.N, g.F, false, g.intraview, B) > ws_bytes) return RLAP_E_WORKSPACE;
    if (const int rc = prepass(st, g, B)) return rc;
    PairMain m{};
    m.own_frag = B.a_frag; m.str_frag = B.b_frag; m.itf = infonce::inv_tau_f(g.tau);
    m.N = g.N; m.Np = infonce::padded_rows(g.N); m.T = infonce::num_tiles(g.N);
    m.groups = (int)infonce::pair_groups(g.N); m.Fp = infonce::padded_features(g.F); m.span = (int)infonce::pair_span_tiles(g.N);
    m.zpart = B.zpart; m.colpart = B.colpart; m.sdiag = B.sdiag;
    const int parts = (int)infonce::pair_parts(g.N);
    const size_t lds = infonce_pair_lds_bytes(g.N, g.F);
    if (const int rc = tile32::allow_lds(&k_in_pair_main, lds)) return rc;
    hipLaunchKernelGGL(k_in_pair_main, dim3((unsigned)(m.groups * parts)), dim3(IN_THREADS), lds, st, m);
    const double c = infonce::positive_coef((g.flags & RLAP_INFONCE_POSITIVE_RAW) != 0, g.tau), itau = infonce::inv_tau(g.tau);
    if (g.intraview != infonce::INTRA_NONE) {   // each view against itself, over the one-direction parts
        const Main im = main_args(g);
        if (const int rc = launch_forward_intra(st, im, g.intraview, B.a_frag, B.zintra)) return rc;
        if (const int rc = launch_forward_intra(st, im, g.intraview, B.b_frag, B.zintra + (int64_t)im.parts * im.Np)) return rc;
        hipLaunchKernelGGL(k_in_pair_rows_intra, dim3(in_blocks(g.N, 256)), dim3(256), 0, st, (const double*)B.zpart, (const double*)B.colpart,
                           (const double*)B.zintra, (const float*)B.sdiag, g.N, m.Np, parts, m.groups, im.parts, c, itau, g.z, g.rows);
    } else {
        hipLaunchKernelGGL(k_in_pair_rows, dim3(in_blocks(g.N, 256)), dim3(256), 0, st, (const double*)B.zpart, (const double*)B.colpart,
                           (const float*)B.sdiag, g.N, m.Np, parts, m.groups, c, itau, g.z, g.rows);
    }
    hipLaunchKernelGGL(k_in_pair_chunks, dim3(in_blocks(2 * spmm::num_chunks(g.N), 256)), dim3(256), 0, st, (const double*)g.rows, g.N, B.csum);
    hipLaunchKernelGGL(k_in_pair_loss, dim3(1), dim3(64), 0, st, (const double*)B.csum, g.N, g.loss);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int infonce_pair_backward_run(hipStream_t st, void* ws, size_t ws_bytes, const InfonceArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_pair(C, g.N, g.F, true, g.intraview, B) > ws_bytes) return RLAP_E_WORKSPACE;
    if (const int rc = prepass(st, g, B)) return rc;
    Main m = main_args(g);
    hipLaunchKernelGGL(k_in_recip, dim3(in_blocks(m.Np, 256)), dim3(256), 0, st, g.z_in, g.N, m.Np, B.rz);             // 1 / Z of the anchors
    hipLaunchKernelGGL(k_in_recip, dim3(in_blocks(m.Np, 256)), dim3(256), 0, st, g.z_in + g.N, g.N, m.Np, B.rz2);     // 1 / Zc of the samples
    RLAP_HIPCHK(hipGetLastError());
    const double c2 = infonce::pair_positive_coef((g.flags & RLAP_INFONCE_POSITIVE_RAW) != 0, g.tau), itau = infonce::inv_tau(g.tau);
    // the anchors own, the samples stream: D = sum_j w_ij bh_j
    const bool intra = g.intraview != infonce::INTRA_NONE;   // then the owner's own view, into the same accumulator
    m.mask_diag = g.intraview == infonce::INTRA_MASKED;
    m.own_frag = B.a_frag; m.str_frag = B.b_frag; m.str_rows = B.b_rows; m.partial = B.part_a; m.rz = B.rz; m.rz2 = B.rz2; m.own_rows = B.a_rows;
    if (const int rc = intra ? launch_backward_main<IN_BACK_PAIR_INTRA>(st, m) : launch_backward_main<IN_BACK_PAIR>(st, m)) return rc;
    // the samples own, the anchors stream: D' = sum_i w_ij ah_i
    m.own_frag = B.b_frag; m.str_frag = B.a_frag; m.str_rows = B.a_rows; m.partial = B.part_b; m.rz = B.rz2; m.rz2 = B.rz; m.own_rows = B.b_rows;
    if (const int rc = intra ? launch_backward_main<IN_BACK_PAIR_INTRA>(st, m) : launch_backward_main<IN_BACK_PAIR>(st, m)) return rc;
    hipLaunchKernelGGL(k_in_grad, dim3(in_blocks(g.N, IN_GRAD_WAVES)), dim3(64 * IN_GRAD_WAVES), 0, st, (const float*)B.part_a, m.parts, g.N, g.F, m.Np, m.Fp,
                       (const float*)B.a_rows, (const float*)B.b_rows, (const double*)B.n2a, g.g, c2, itau, 1, g.ga);
    hipLaunchKernelGGL(k_in_grad, dim3(in_blocks(g.N, IN_GRAD_WAVES)), dim3(64 * IN_GRAD_WAVES), 0, st, (const float*)B.part_b, m.parts, g.N, g.F, m.Np, m.Fp,
                       (const float*)B.b_rows, (const float*)B.a_rows, (const double*)B.n2b, g.g, c2, itau, 1, g.gb);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace rlap
