// rlap_linear.hip -- the fused dense layer, forward and backward (rlap_linear_act / rlap_linear_act_backward):
// y = act(x W + b) in one pass over x, and gx, gW, gb from (x, W, y, gy).  Every product comes from v_mfma_f32_32x32x2_f32 -- bit
// for bit a k-ordered float32 fmaf chain --; every sum has the fixed order of rlap_linear.h.  A translation unit of its own.
//
//   weight      the padded image of W in the arena, (Finp, Foutp) for the forward product and (Foutp, Finp) for the input gradient,
//               from either layout of W: the only operand that is copied (at most 1 MiB).
//   product     the z r product of rlap_bt.hip made rectangular: a 32-row tile of the A operand read IN PLACE from x (forward) or
//               formed from gy and y while it is loaded (input gradient), rows >= M and columns >= K as zeros; 32 rows of the
//               weight image staged through LDS as B, the next 32 and the next slab's A operands fetched into registers
//               meanwhile; the bias, the activation and the rounding applied to the accumulator registers, y written straight
//               from them with rows >= M and columns >= C left alone.  The work map is the header's (col_waves, row_tiles,
//               product_instance).
//   weight grad the rectangular form of k_bt_cross: 32 rows x 64 columns of x and 32 rows x 64 NW columns of t staged in LDS through
//               guarded loads, wave w owning the super-tile pair (I, J0 + w); one partial tile per part, the parts added in float64
//               in part order by k_lin_gwfinish, which writes gW in W's layout.
//   bias grad   the column sums of t by the chunk rule, a pass of its own: chunk sums, then their sum in chunk order.
// No float atomics, no host synchronisation, nothing allocated outside the arena, no padded copy of x, y, gy or gx.  The lane
// path (16-byte or 4-byte loads of the rows) is linear::vec_ok of the shape and the base pointers; both give the same bits.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/rlap_hip.h"
#include "rlap_linear.h"
#include "rlap_linear_api.h"
#include "rlap_spmm.h"
#include "rlap_tile32_dev.h"

namespace rlap {
namespace {

using tile32::f32x16;
typedef float f32x4 __attribute__((ext_vector_type(4)));   // 16 bytes of a row

constexpr int LIN_THREADS = 256;                // four waves
constexpr int64_t LIN_MAX_GRID = 1 << 20;       // workgroups of a striding launch
constexpr int LIN_A_COLS = 64;                  // columns of the staged slab of x in the weight gradient: one super tile
static_assert(LIN_THREADS == 64 * linear::WAVES && linear::WAVES == linear::GROUP_PAIRS, "one wave per super-tile pair");
static_assert(linear::SUPER == 2 && LIN_A_COLS == linear::SUPER * linear::TILE, "the weight gradient holds 2 x 2 accumulator tiles");

inline unsigned lin_blocks(int64_t n, int per_block) { return capped_blocks(n, per_block, LIN_MAX_GRID); }

enum { MODE_FORWARD = 0, MODE_GX = 1 };

// ------------------------------------------------------------------------------------------------ the padded weight images
// image (Kp, Cp) of the weight: transposed == 0: rows k of Fin, columns o of Fout; transposed != 0: rows o, columns k
__global__ __launch_bounds__(256) void k_lin_wpad(const float* __restrict__ w, int Fin, int Fout, int flags, int transposed, int Kp, int Cp,
                                                  float* __restrict__ wp) {
    const int64_t ee = (int64_t)Kp * Cp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ee; e += (int64_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / Cp), c = (int)(e - (int64_t)r * Cp);
        const int k = transposed ? c : r, o = transposed ? r : c;
        wp[e] = (k < Fin && o < Fout) ? w[linear::weight_index(k, o, Fin, Fout, flags)] : 0.0f;
    }
}

// ------------------------------------------------------------------------------------------------ guarded loads of the operands
// four consecutive elements of row `row` from column `col` (a multiple of 4) of an (M, F) array: zeros behind M and F
template <bool VEC>
__device__ __forceinline__ f32x4 lin_load4(const float* __restrict__ p, int64_t row, int col, int64_t M, int F) {
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (row >= M) return v;
    const float* q = p + row * F + col;
    if (VEC) {                                   // (F % 4 == 0: col < F means col + 3 < F)
        if (col < F) v = *reinterpret_cast<const f32x4*>(q);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (col + e < F) v[e] = q[e];
    }
    return v;
}

// the same of t, formed from gy and y
template <bool VEC>
__device__ __forceinline__ f32x4 lin_load4_t(const float* __restrict__ gy, const float* __restrict__ y, int64_t row, int col, int64_t M, int F,
                                             int act, double alpha) {
    const f32x4 g = lin_load4<VEC>(gy, row, col, M, F);
    if (act == linear::ACT_NONE) return g;       // (t = (float)((double)gy * 1) = gy)
    const f32x4 yv = lin_load4<VEC>(y, row, col, M, F);
    f32x4 t;
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = linear::t_of(g[e], yv[e], act, alpha);
    return t;
}

// ------------------------------------------------------------------------------------------------ the product
struct Prod {
    const float* a0; const float* a1;               // forward: x, -; input gradient: gy, y -- (M, K) each, read in place
    const float* wp;                                // the weight image (Kp, Cp)
    const float* bias;                              // forward: (C,) or null
    int64_t M; int K, C, Kp, Cp, nct;
    int act; double alpha;
    float* out;                                     // (M, C), written in place
};

// a workgroup is linear::row_tiles(nct) = 4 / CW row tiles; wave w works on row tile w / CW of them and owns the column tiles
// w % CW + CW j, j < NCT
template <int CW, int NCT, int MODE, bool VEC>
__global__ __launch_bounds__(LIN_THREADS) void k_lin_product(Prod a) {
    extern __shared__ __attribute__((aligned(16))) float lin_lds[];  // 32 x Cp floats: rows l0 .. l0 + 31 of the weight image
    constexpr int NPRE = CW * NCT;                                   // (>= nct float4s a thread of a 32-row slab)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    const int64_t tile = linear::wave_row_tile(blockIdx.x, wave, a.nct);
    const int64_t row = tile * linear::TILE + c;                     // the lane's row of the A operand (guarded: may be >= M)
    const float* __restrict__ a0 = a.a0;
    const float* __restrict__ a1 = a.a1;
    float4 pre[NPRE];
    const float4* __restrict__ wsrc = reinterpret_cast<const float4*>(a.wp) + threadIdx.x;
    const int row_vec = a.Cp >> 2;

    f32x16 acc[NCT];
#pragma unroll
    for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

    // columns l0 + 4 q .. l0 + 4 q + 3 of the lane's row, q < 8: the A operands of a slab, fetched one slab ahead as the weight is
    f32x4 an[linear::TILE / 4];
    const auto fetch_a = [&](int l0) {
#pragma unroll
        for (int q = 0; q < linear::TILE / 4; ++q)
            an[q] = MODE == MODE_FORWARD ? lin_load4<VEC>(a0, row, l0 + 4 * q, a.M, a.K)
                                         : lin_load4_t<VEC>(a0, a1, row, l0 + 4 * q, a.M, a.K, a.act, a.alpha);
    };

#pragma unroll
    for (int j = 0; j < NPRE; ++j) pre[j] = j < a.nct ? wsrc[j * LIN_THREADS] : float4{0.0f, 0.0f, 0.0f, 0.0f};
    fetch_a(0);
#pragma unroll 1
    for (int l0 = 0; l0 < a.Kp; l0 += linear::TILE) {
        __syncthreads();
        {
            float4* dst = reinterpret_cast<float4*>(lin_lds) + threadIdx.x;
#pragma unroll
            for (int j = 0; j < NPRE; ++j)
                if (j < a.nct) dst[j * LIN_THREADS] = pre[j];
        }
        __syncthreads();
        if (l0 + linear::TILE < a.Kp) {                              // in flight while this slab is multiplied
#pragma unroll
            for (int j = 0; j < NPRE; ++j)
                if (j < a.nct) pre[j] = wsrc[(l0 + linear::TILE) * row_vec + j * LIN_THREADS];
        }
        f32x4 cur[linear::TILE / 4];
#pragma unroll
        for (int q = 0; q < linear::TILE / 4; ++q) cur[q] = an[q];
        if (l0 + linear::TILE < a.Kp) fetch_a(l0 + linear::TILE);    // (wave-uniform)
        const float* brow = lin_lds + h * a.Cp + c;
#pragma unroll
        for (int q = 0; q < linear::TILE / 4; ++q) {                 // columns l0 + 4 q .. l0 + 4 q + 3 of the lane's row: steps 2 q, 2 q + 1
            const f32x4 v = cur[q];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int s = 2 * q + u;
                const float av = u ? (h ? v[3] : v[2]) : (h ? v[1] : v[0]);   // A[row][l0 + 2 s + h]
#pragma unroll
                for (int j = 0; j < NCT; ++j) {
                    const int ct = (wave % CW) + CW * j;
                    if (ct < a.nct) {                                // (wave-uniform)
                        const float bv = brow[2 * s * a.Cp + ct * linear::TILE];
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
                    }
                }
            }
        }
    }

    const bool has_bias = MODE == MODE_FORWARD && a.bias != nullptr;
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
        const int ct = (wave % CW) + CW * j;
        const int col = ct * linear::TILE + c;
        if (ct < a.nct && col < a.C) {
            const float bias = has_bias ? a.bias[col] : 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t orow = tile * linear::TILE + linear::reg_row(r, h);
                if (orow < a.M)
                    a.out[orow * a.C + col] = MODE == MODE_FORWARD ? linear::y_of(acc[j][r], has_bias, bias, a.act, a.alpha) : acc[j][r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ the weight gradient
struct Cross {
    const float* x; const float* gy; const float* y;
    int64_t M; int Fin, Fout, Finp, Foutp, nft_in, nft_out, nst_out, rgroups, groups, parts;
    int act; double alpha;
    float* partial;                                 // [parts, Finp, Foutp]: every tile is written
};

template <int NW, bool VEC>
__device__ __forceinline__ void lin_fetch(f32x4 (&pa)[2], f32x4 (&pb)[2 * NW], const Cross& a, int64_t row, int I, int J0, int tid) {
    constexpr int AV = LIN_A_COLS / 4, BV = 16 * NW;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int v = tid + LIN_THREADS * j;
        pa[j] = lin_load4<VEC>(a.x, row + v / AV, LIN_A_COLS * I + 4 * (v % AV), a.M, a.Fin);
    }
#pragma unroll
    for (int j = 0; j < 2 * NW; ++j) {
        const int v = tid + LIN_THREADS * j;
        pb[j] = lin_load4_t<VEC>(a.gy, a.y, row + v / BV, LIN_A_COLS * J0 + 4 * (v % BV), a.M, a.Fout, a.act, a.alpha);
    }
}

// NW: the 64-column super tiles of t a workgroup stages (its waves' pairs)
template <int NW, bool VEC>
__global__ __launch_bounds__(LIN_THREADS) void k_lin_cross(Cross a) {
    constexpr int BW = 64 * NW;                                      // columns of the slab of t
    __shared__ __attribute__((aligned(16))) float s_a[linear::TILE * LIN_A_COLS];
    __shared__ __attribute__((aligned(16))) float s_b[linear::TILE * BW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    const int grp = (int)(blockIdx.x % a.groups);
    const int part = (int)(blockIdx.x / a.groups);                   // (< parts: the grid is parts * groups)
    int I, J0;
    linear::group_of(grp, a.rgroups, &I, &J0);
    const bool active = wave < NW && linear::wave_active(J0, wave, a.nst_out);   // (wave-uniform)
    const int J = active ? J0 + wave : J0;
    // the columns of the wave's four operands inside the staged slabs (a clamped tile is inside too)
    const int ka0 = linear::tile_of(I, 0, a.nft_in) * linear::TILE - LIN_A_COLS * I, ka1 = linear::tile_of(I, 1, a.nft_in) * linear::TILE - LIN_A_COLS * I;
    const int kb0 = linear::tile_of(J, 0, a.nft_out) * linear::TILE - LIN_A_COLS * J0, kb1 = linear::tile_of(J, 1, a.nft_out) * linear::TILE - LIN_A_COLS * J0;
    const int64_t r0 = linear::part_begin(a.M, a.Fin, a.Fout, part), r1 = linear::part_begin(a.M, a.Fin, a.Fout, part + 1);
    const int tid = threadIdx.x;
    f32x4 pa[2], pb[2 * NW];

    f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc00[r] = 0.0f; acc01[r] = 0.0f; acc10[r] = 0.0f; acc11[r] = 0.0f; }

    lin_fetch<NW, VEC>(pa, pb, a, r0, I, J0, tid);                   // (a part is never empty)
#pragma unroll 1
    for (int64_t row = r0; row < r1; row += linear::TILE) {
        __syncthreads();   // (the previous rows have been read)
#pragma unroll
        for (int j = 0; j < 2; ++j) reinterpret_cast<f32x4*>(s_a)[tid + LIN_THREADS * j] = pa[j];
#pragma unroll
        for (int j = 0; j < 2 * NW; ++j) reinterpret_cast<f32x4*>(s_b)[tid + LIN_THREADS * j] = pb[j];
        __syncthreads();
        if (row + linear::TILE < r1) lin_fetch<NW, VEC>(pa, pb, a, row + linear::TILE, I, J0, tid);   // in flight while this step is multiplied
        if (active) {
            const float* qa = s_a + h * LIN_A_COLS + c;              // row (2 s + h) of the step, the lane's column of a tile
            const float* qb = s_b + h * BW + c;
#pragma unroll 4
            for (int s = 0; s < linear::TILE / 2; ++s) {
                const float a0 = qa[2 * s * LIN_A_COLS + ka0], a1 = qa[2 * s * LIN_A_COLS + ka1];
                const float b0 = qb[2 * s * BW + kb0], b1 = qb[2 * s * BW + kb1];
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
            }
        }
    }

    if (!active) return;
    float* __restrict__ out = a.partial + (int64_t)part * a.Finp * a.Foutp;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int ta = t >> 1, tb = t & 1;
        if (!linear::tile_stored(I, J, ta, tb, a.nft_in, a.nft_out)) continue;   // (wave-uniform)
        const f32x16& acc = t == 0 ? acc00 : (t == 1 ? acc01 : (t == 2 ? acc10 : acc11));
        const int k0 = (linear::SUPER * I + ta) * linear::TILE, l0 = (linear::SUPER * J + tb) * linear::TILE;
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(k0 + linear::reg_row(r, h)) * a.Foutp + l0 + c] = acc[r];
    }
}

// gW_ko = (float)(the parts in order, in float64), written in W's layout
__global__ __launch_bounds__(256) void k_lin_gwfinish(const float* __restrict__ partial, int parts, int Fin, int Fout, int Finp, int Foutp,
                                                      int flags, float* __restrict__ gw) {
    const int64_t ee = (int64_t)Fin * Fout;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ee; e += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / Fout), o = (int)(e - (int64_t)k * Fout);
        double S = 0.0;
        for (int p = 0; p < parts; ++p) S = S + (double)partial[((int64_t)p * Finp + k) * Foutp + o];
        gw[linear::weight_index(k, o, Fin, Fout, flags)] = (float)S;
    }
}

// ------------------------------------------------------------------------------------------------ the bias gradient
struct Gb {
    const float* gy; const float* y; int64_t M; int Fout; int act; double alpha;
    double* cs;                                     // [num_chunks(M), Fout] chunk sums
    float* gb;
};

__global__ __launch_bounds__(256) void k_lin_gbchunks(Gb a) {
    const int64_t nc = spmm::num_chunks(a.M), ncb = (a.Fout + 255) / 256;
    for (int64_t item = blockIdx.x; item < nc * ncb; item += gridDim.x) {
        const int64_t chunk = item / ncb;
        const int col = (int)(item - chunk * ncb) * 256 + (int)threadIdx.x;
        if (col >= a.Fout) continue;
        double s = 0.0;
        for (int64_t i = spmm::chunk_begin(chunk); i < spmm::chunk_end(a.M, chunk); ++i) {
            const float g = a.gy[i * a.Fout + col];
            const float t = a.act == linear::ACT_NONE ? g : linear::t_of(g, a.y[i * a.Fout + col], a.act, a.alpha);
            s = spmm::accumulate(s, 1.0, (double)t);
        }
        a.cs[chunk * a.Fout + col] = s;
    }
}

__global__ __launch_bounds__(256) void k_lin_gbfinish(Gb a) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= a.Fout) return;
    const int64_t nc = spmm::num_chunks(a.M);
    double total = 0.0;
    for (int64_t k0 = 0; k0 < nc; k0 += 8) {   // eight loads in flight, added in chunk order
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = k0 + j < nc ? a.cs[(k0 + j) * a.Fout + col] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k0 + j < nc) total = total + t[j];
    }
    a.gb[col] = (float)total;
}

// ------------------------------------------------------------------------------------------------ host
struct Bufs {
    float* wp;                                      // forward: (Finp, Foutp); backward with gx: (Foutp, Finp)
    float* partial; double* cs;                     // backward with gw; with gb
};

size_t carve_linear(Carve& C, int64_t M, int64_t Fin, int64_t Fout, bool backward, bool gx, bool gw, bool gb, Bufs& B) {
    const int64_t Finp = linear::padded_features(Fin), Foutp = linear::padded_features(Fout);
    B = Bufs{};
    if (!backward || gx) B.wp = C.take<float>(Finp * Foutp);
    if (backward && gw) B.partial = C.take<float>(linear::num_parts(M, Fin, Fout) * Finp * Foutp);
    if (backward && gb) B.cs = C.take<double>(spmm::num_chunks(M) * Fout);
    return C.off + 256;
}

uint64_t bits_of(const void* p) { return (uint64_t)reinterpret_cast<uintptr_t>(p); }

template <int CW, int NCT, int MODE>
int launch_product(hipStream_t st, const Prod& a, bool vec) {
    const size_t lds = (size_t)linear::TILE * a.Cp * sizeof(float);
    const dim3 grid((unsigned)linear::product_groups(a.M, a.nct));
    if (vec) {
        if (const int rc = tile32::allow_lds(&k_lin_product<CW, NCT, MODE, true>, lds)) return rc;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_product<CW, NCT, MODE, true>), grid, dim3(LIN_THREADS), lds, st, a);
    } else {
        if (const int rc = tile32::allow_lds(&k_lin_product<CW, NCT, MODE, false>, lds)) return rc;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_product<CW, NCT, MODE, false>), grid, dim3(LIN_THREADS), lds, st, a);
    }
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// the instance by the header's rules; no instance (a width outside [1, MAX_F], which the entry points refuse) is an error
template <int MODE>
int launch_product_of(hipStream_t st, const Prod& a, bool vec) {
    const int cw = linear::col_waves(a.nct);
    switch (linear::product_instance(a.nct)) {
        case 1: return cw == 1 ? launch_product<1, 1, MODE>(st, a, vec) : (cw == 2 ? launch_product<2, 1, MODE>(st, a, vec) : launch_product<4, 1, MODE>(st, a, vec));
        case 2: return launch_product<4, 2, MODE>(st, a, vec);
        case 3: return launch_product<4, 3, MODE>(st, a, vec);
        case 4: return launch_product<4, 4, MODE>(st, a, vec);
    }
    return RLAP_E_INTERNAL;
}

template <int NW>
int launch_cross(hipStream_t st, const Cross& m, bool vec) {
    const dim3 grid((unsigned)(m.parts * m.groups));
    if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_cross<NW, true>), grid, dim3(LIN_THREADS), 0, st, m);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_lin_cross<NW, false>), grid, dim3(LIN_THREADS), 0, st, m);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int launch_cross_of(hipStream_t st, const Cross& m, bool vec) {
    switch (linear::cross_instance(m.nft_out)) {
        case 1: return launch_cross<1>(st, m, vec);
        case 2: return launch_cross<2>(st, m, vec);
        case 4: return launch_cross<4>(st, m, vec);
    }
    return RLAP_E_INTERNAL;
}

int launch_wpad(hipStream_t st, const LinearArgs& g, int transposed, float* wp) {
    const int Finp = linear::padded_features(g.Fin), Foutp = linear::padded_features(g.Fout);
    const int Kp = transposed ? Foutp : Finp, Cp = transposed ? Finp : Foutp;
    hipLaunchKernelGGL(k_lin_wpad, dim3(lin_blocks((int64_t)Kp * Cp, 256)), dim3(256), 0, st, g.w, (int)g.Fin, (int)g.Fout, g.flags, transposed, Kp, Cp, wp);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace

size_t linear_bytes(int64_t M, int64_t Fin, int64_t Fout) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_linear(C, M, Fin, Fout, false, false, false, false, B);
}

size_t linear_backward_bytes(int64_t M, int64_t Fin, int64_t Fout, bool gx, bool gw, bool gb) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_linear(C, M, Fin, Fout, true, gx, gw, gb, B);
}

int linear_run(hipStream_t st, void* ws, size_t ws_bytes, const LinearArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_linear(C, g.M, g.Fin, g.Fout, false, false, false, false, B) > ws_bytes) return RLAP_E_WORKSPACE;
    if (const int rc = launch_wpad(st, g, 0, B.wp)) return rc;
    Prod a{};
    a.a0 = g.x; a.wp = B.wp; a.bias = g.b; a.M = g.M; a.K = (int)g.Fin; a.C = (int)g.Fout;
    a.Kp = linear::padded_features(g.Fin); a.Cp = linear::padded_features(g.Fout); a.nct = linear::feature_tiles(g.Fout);
    a.act = g.act; a.alpha = g.alpha; a.out = g.y;
    return launch_product_of<MODE_FORWARD>(st, a, linear::vec_ok(g.Fin, bits_of(g.x)));
}

int linear_backward_run(hipStream_t st, void* ws, size_t ws_bytes, const LinearArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_linear(C, g.M, g.Fin, g.Fout, true, g.gx != nullptr, g.gw != nullptr, g.gb != nullptr, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const bool vec_t = linear::vec_ok(g.Fout, bits_of(g.gy) | bits_of(g.y_in));
    if (g.gx) {
        if (const int rc = launch_wpad(st, g, 1, B.wp)) return rc;
        Prod a{};
        a.a0 = g.gy; a.a1 = g.y_in; a.wp = B.wp; a.M = g.M; a.K = (int)g.Fout; a.C = (int)g.Fin;
        a.Kp = linear::padded_features(g.Fout); a.Cp = linear::padded_features(g.Fin); a.nct = linear::feature_tiles(g.Fin);
        a.act = g.act; a.alpha = g.alpha; a.out = g.gx;
        if (const int rc = launch_product_of<MODE_GX>(st, a, vec_t)) return rc;
    }
    if (g.gw) {
        Cross m{};
        m.x = g.x; m.gy = g.gy; m.y = g.y_in; m.M = g.M; m.Fin = (int)g.Fin; m.Fout = (int)g.Fout;
        m.Finp = linear::padded_features(g.Fin); m.Foutp = linear::padded_features(g.Fout);
        m.nft_in = linear::feature_tiles(g.Fin); m.nft_out = linear::feature_tiles(g.Fout); m.nst_out = linear::super_tiles(g.Fout);
        m.rgroups = linear::row_groups(g.Fout); m.groups = linear::pair_groups(g.Fin, g.Fout);
        m.parts = (int)linear::num_parts(g.M, g.Fin, g.Fout); m.act = g.act; m.alpha = g.alpha; m.partial = B.partial;
        if (const int rc = launch_cross_of(st, m, vec_t && linear::vec_ok(g.Fin, bits_of(g.x)))) return rc;
        hipLaunchKernelGGL(k_lin_gwfinish, dim3(lin_blocks(g.Fin * g.Fout, 256)), dim3(256), 0, st, (const float*)B.partial, m.parts, m.Fin, m.Fout,
                           m.Finp, m.Foutp, g.flags, g.gw);
        RLAP_HIPCHK(hipGetLastError());
    }
    if (g.gb) {
        Gb b{g.gy, g.y_in, g.M, (int)g.Fout, g.act, g.alpha, B.cs, g.gb};
        const int64_t items = spmm::num_chunks(g.M) * ((g.Fout + 255) / 256);
        hipLaunchKernelGGL(k_lin_gbchunks, dim3(lin_blocks(items, 1)), dim3(256), 0, st, b);
        hipLaunchKernelGGL(k_lin_gbfinish, dim3((unsigned)((g.Fout + 255) / 256)), dim3(256), 0, st, b);
        RLAP_HIPCHK(hipGetLastError());
    }
    return RLAP_OK;
}

}  // namespace rlap
