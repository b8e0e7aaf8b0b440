// rlap_bt.hip -- the fused Barlow Twins loss, forward and backward (rlap_bt_loss / rlap_bt_loss_backward): the
// standardisation and the loss of PyGCL's bt_loss on two views' embeddings.  The cross product z1^T z2 is a tall-skinny product over
// the node index and comes from v_mfma_f32_32x32x2_f32 -- bit for bit a k-ordered float32 fmaf chain --; every sum has the fixed
// order of rlap_bt.h.  A translation unit of its own; the pattern of its pre-pass, finish and backward is rlap_cca.hip's
// (DESIGN 4.16), restated here so that that unit's code stays as it is.
//
//   pre-pass   the column statistics in float64 by the chunk rule, in two passes, as in rlap_cca.hip; the standardised copies z1, z2
//              in the arena, row-major, zero-padded to 32-row tiles and to a multiple of 32 columns.  With NO_STANDARDIZE the
//              copies are the inputs and no statistics are taken.
//   cross      work is (part of the rows, block row I of super tiles, group of four block columns J0 .. J0 + 3).  A workgroup of
//              four waves stages 32 rows x 64 columns of z1 and 32 rows x 64 NW columns of z2 in LDS (40 KB at NW = 4), the next
//              32 rows being fetched into registers meanwhile; wave w OWNS pair (I, J0 + w), 2 x 2 accumulator tiles (64
//              registers), and per row pair reads two A operands (z1) and two B operands (z2) from LDS for four MFMAs.  Every tile
//              of the full nft x nft grid is stored, one partial tile per part.
//   finish     the part tiles added in part order in float64, c = S / N, cross = (float)c; the chunk sums of the off-diagonal and
//              of the diagonal terms; the three terms by one workgroup.
//   backward   z again from h and the forward's column statistics; W^T and W padded with zeros; P1 = z2 W^T and P2 = z1 W by the
//              z r product of rlap_cca.hip (a 32-row tile of z as the A operand, 32 rows of the weight staged through LDS as B);
//              then the two column sums of dz by the chunk rule and the dh pass, dz formed from P wherever it is read.
// No float atomics, no host synchronisation, nothing allocated outside the arena.  Every address is formed from the padded sizes.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/rlap_hip.h"
#include "rlap_bt.h"
#include "rlap_bt_api.h"
#include "rlap_spmm.h"
#include "rlap_tile32_dev.h"

namespace rlap {
namespace {

using tile32::f32x16;
typedef float f32x4 __attribute__((ext_vector_type(4)));   // 16 bytes of a staged row

constexpr int BT_THREADS = 256;                 // four waves: bt::GROUP_PAIRS super-tile pairs
constexpr int64_t BT_MAX_GRID = 1 << 20;        // workgroups of a striding launch
constexpr int BT_A_COLS = 64;                   // columns of the staged slab of z1: one super tile
static_assert(BT_THREADS == 64 * bt::GROUP_PAIRS, "one wave per super-tile pair");
static_assert(bt::SUPER == 2 && BT_A_COLS == bt::SUPER * bt::TILE, "the cross kernel holds 2 x 2 accumulator tiles");

inline unsigned bt_blocks(int64_t n, int per_block) { return capped_blocks(n, per_block, BT_MAX_GRID); }

// ------------------------------------------------------------------------------------------------ column sums by the chunk rule
enum { CS_SUM = 0, CS_SS = 1, CS_M = 2, CS_Q = 3 };

struct Col {
    const float* h[2]; int64_t N; int F;            // the inputs (CS_SUM, CS_SS)
    const float* z[2]; const float* P[2]; int Fp;   // the padded images (CS_M, CS_Q): z[v] and P[v] belong to view v
    const double* colstat;                          // mean1 | sd1 | mean2 | sd2
    const double* g; double eps;                    // backward: the upstream gradient
    int ncols;                                      // 2 F
    double* cs;                                     // [num_chunks(N), ncols] chunk sums
    double* out;                                    // what the finish writes (see k_bt_colfinish)
};

// the term (c, x) of row i of column c of the list a mode sums
template <int MODE>
__device__ inline void bt_term(const Col& a, int64_t i, int col, double g, double* c, double* x) {
    const int v = col >= a.F ? 1 : 0, k = col - v * a.F;
    if (MODE == CS_SUM) {
        *c = 1.0; *x = (double)a.h[v][i * a.F + k];
    } else if (MODE == CS_SS) {
        const double d = cca::centred(a.h[v][i * a.F + k], a.colstat[v * 2 * a.F + k]);
        *c = d; *x = d;
    } else {
        const double dz = bt::dz_of(g, a.P[v][i * a.Fp + k], a.N);
        if (MODE == CS_M) { *c = 1.0; *x = dz; } else { *c = dz; *x = (double)a.z[v][i * a.Fp + k]; }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_bt_colchunks(Col a) {
    const int64_t nc = spmm::num_chunks(a.N), ncb = (a.ncols + 255) / 256;
    const double g = (MODE == CS_M || MODE == CS_Q) ? *a.g : 0.0;
    for (int64_t item = blockIdx.x; item < nc * ncb; item += gridDim.x) {
        const int64_t chunk = item / ncb;
        const int col = (int)(item - chunk * ncb) * 256 + (int)threadIdx.x;
        if (col >= a.ncols) continue;
        double s = 0.0;
        for (int64_t i = spmm::chunk_begin(chunk); i < spmm::chunk_end(a.N, chunk); ++i) {
            double c, x;
            bt_term<MODE>(a, i, col, g, &c, &x);
            s = spmm::accumulate(s, c, x);
        }
        a.cs[chunk * a.ncols + col] = s;
    }
}

// the chunk sums of a column added in order; out: CS_SUM the means and CS_SS the deviations of colstat's layout, CS_M m [2 F],
// CS_Q q [2 F]
template <int MODE>
__global__ __launch_bounds__(256) void k_bt_colfinish(Col a) {
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= a.ncols) return;
    const int64_t nc = spmm::num_chunks(a.N);
    double total = 0.0;
    for (int64_t k0 = 0; k0 < nc; k0 += 8) {   // eight loads in flight, added in chunk order
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = k0 + j < nc ? a.cs[(k0 + j) * a.ncols + col] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (k0 + j < nc) total = total + t[j];
    }
    const int v = col >= a.F ? 1 : 0, k = col - v * a.F;
    if (MODE == CS_SUM) a.out[v * 2 * a.F + k] = cca::col_mean(total, a.N);
    else if (MODE == CS_SS) a.out[v * 2 * a.F + a.F + k] = cca::col_sd(total, a.N);
    else if (MODE == CS_M) a.out[col] = bt::col_m(total, a.N);
    else a.out[col] = bt::col_q(total, a.N);
}

template <int MODE>
int col_sums(hipStream_t st, const Col& a) {
    const int64_t items = spmm::num_chunks(a.N) * ((a.ncols + 255) / 256);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_colchunks<MODE>), dim3(bt_blocks(items, 1)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_colfinish<MODE>), dim3((unsigned)((a.ncols + 255) / 256)), dim3(256), 0, st, a);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// the standardised copies of both views (or, with `plain`, the inputs themselves), padded with zeros: z[v] is Np x Fp
__global__ __launch_bounds__(256) void k_bt_z(const float* __restrict__ h0, const float* __restrict__ h1, const double* __restrict__ colstat,
                                              double eps, int plain, int64_t N, int F, int64_t Np, int Fp, float* __restrict__ z0,
                                              float* __restrict__ z1) {
    const int64_t elems = Np * Fp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * elems; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = e >= elems ? 1 : 0;
        const int64_t w = e - v * elems, i = w / Fp;
        const int k = (int)(w - i * Fp);
        float val = 0.0f;
        if (i < N && k < F) {
            const float x = (v ? h1 : h0)[i * F + k];
            val = plain ? x : bt::zval(x, colstat[v * 2 * F + k], bt::scale_of(colstat[v * 2 * F + F + k], eps));
        }
        (v ? z1 : z0)[w] = val;
    }
}

// ------------------------------------------------------------------------------------------------ the cross product
struct Cross {
    const float* z1; const float* z2;
    int64_t N; int F, Fp, nft, nst, rgroups, groups, parts;
    float* partial;                                 // [parts, Fp, Fp]: every tile is written
};

// the float4s a thread stages of the 32 rows from `row`: float4 v = tid + 256 j of a slab lies in row v / (float4s of a row), at the
// columns behind it; a column >= Fp is not read
template <int NW>
__device__ __forceinline__ void bt_fetch(f32x4 (&pa)[2], f32x4 (&pb)[2 * NW], const float* __restrict__ z1, const float* __restrict__ z2,
                                         int64_t row, int Fp, int I, int J0, int tid) {
    constexpr int AV = BT_A_COLS / 4, BV = 16 * NW;
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int v = tid + BT_THREADS * j, col = BT_A_COLS * I + 4 * (v % AV);
        pa[j] = col < Fp ? *reinterpret_cast<const f32x4*>(z1 + (row + v / AV) * Fp + col) : zero4;
    }
#pragma unroll
    for (int j = 0; j < 2 * NW; ++j) {
        const int v = tid + BT_THREADS * j, col = BT_A_COLS * J0 + 4 * (v % BV);
        pb[j] = col < Fp ? *reinterpret_cast<const f32x4*>(z2 + (row + v / BV) * Fp + col) : zero4;
    }
}

// NW: the 64-column super tiles of z2 a workgroup stages (its waves' pairs): 2 NW float4s a thread and step, fetched into
// registers one step ahead, beside the 2 of z1
template <int NW>
__global__ __launch_bounds__(BT_THREADS) void k_bt_cross(Cross a) {
    constexpr int BW = 64 * NW;                                      // columns of the z2 slab
    __shared__ __attribute__((aligned(16))) float s_a[bt::TILE * BT_A_COLS];
    __shared__ __attribute__((aligned(16))) float s_b[bt::TILE * BW];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    const int grp = (int)(blockIdx.x % a.groups);
    const int part = (int)(blockIdx.x / a.groups);                   // (< parts: the grid is parts * groups)
    int I, J0;
    bt::group_of(grp, a.rgroups, &I, &J0);
    const bool active = wave < NW && bt::wave_active(J0, wave, a.nst);   // (wave-uniform)
    const int J = active ? J0 + wave : J0;
    // the columns of the wave's four operands inside the staged slabs (a clamped tile is inside too)
    const int ka0 = bt::tile_of(I, 0, a.nft) * bt::TILE - BT_A_COLS * I, ka1 = bt::tile_of(I, 1, a.nft) * bt::TILE - BT_A_COLS * I;
    const int kb0 = bt::tile_of(J, 0, a.nft) * bt::TILE - BT_A_COLS * J0, kb1 = bt::tile_of(J, 1, a.nft) * bt::TILE - BT_A_COLS * J0;
    const int64_t r0 = bt::part_begin(a.N, a.F, part), r1 = bt::part_begin(a.N, a.F, part + 1);   // (r1 <= the padded rows)
    const float* __restrict__ z1 = a.z1;
    const float* __restrict__ z2 = a.z2;
    const int tid = threadIdx.x;
    f32x4 pa[2], pb[2 * NW];

    f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc00[r] = 0.0f; acc01[r] = 0.0f; acc10[r] = 0.0f; acc11[r] = 0.0f; }

    bt_fetch<NW>(pa, pb, z1, z2, r0, a.Fp, I, J0, tid);               // (a part is never empty)
#pragma unroll 1
    for (int64_t row = r0; row < r1; row += bt::TILE) {
        __syncthreads();   // (the previous rows have been read)
#pragma unroll
        for (int j = 0; j < 2; ++j) reinterpret_cast<f32x4*>(s_a)[tid + BT_THREADS * j] = pa[j];
#pragma unroll
        for (int j = 0; j < 2 * NW; ++j) reinterpret_cast<f32x4*>(s_b)[tid + BT_THREADS * j] = pb[j];
        __syncthreads();
        if (row + bt::TILE < r1) bt_fetch<NW>(pa, pb, z1, z2, row + bt::TILE, a.Fp, I, J0, tid);   // in flight while this step is multiplied
        if (active) {
            const float* qa = s_a + h * BT_A_COLS + c;               // row (2 s + h) of the step, the lane's column of a tile
            const float* qb = s_b + h * BW + c;
#pragma unroll 4
            for (int s = 0; s < bt::TILE / 2; ++s) {
                const float a0 = qa[2 * s * BT_A_COLS + ka0], a1 = qa[2 * s * BT_A_COLS + ka1];
                const float b0 = qb[2 * s * BW + kb0], b1 = qb[2 * s * BW + kb1];
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
            }
        }
    }

    if (!active) return;
    float* __restrict__ out = a.partial + (int64_t)part * a.Fp * a.Fp;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int ta = t >> 1, tb = t & 1;
        if (!bt::tile_stored(I, J, ta, tb, a.nft)) continue;         // (wave-uniform)
        const f32x16& acc = t == 0 ? acc00 : (t == 1 ? acc01 : (t == 2 ? acc10 : acc11));
        const int k0 = (bt::SUPER * I + ta) * bt::TILE, l0 = (bt::SUPER * J + tb) * bt::TILE;
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(k0 + bt::reg_row(r, h)) * a.Fp + l0 + c] = acc[r];
    }
}

// S = the parts in order, c = S / N, cross = (float)c
__global__ __launch_bounds__(256) void k_bt_finish(const float* __restrict__ partial, int parts, int64_t N, int F, int Fp,
                                                   double* __restrict__ C, float* __restrict__ cross) {
    const int64_t ff = (int64_t)F * F;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < ff; e += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / F), l = (int)(e - (int64_t)k * F);
        double S = 0.0;
        for (int p = 0; p < parts; ++p) S = S + (double)partial[((int64_t)p * Fp + k) * Fp + l];
        const double cv = bt::c_of(S, N);
        C[e] = cv;
        cross[e] = (float)cv;
    }
}

// the chunk sums of the off-diagonal terms over the F * F entries, then those of the diagonal terms over k: ocs is
// [num_chunks(F F) + num_chunks(F)]
__global__ __launch_bounds__(256) void k_bt_chunks(const double* __restrict__ C, int F, double* __restrict__ ocs) {
    const int64_t ff = (int64_t)F * F, nc = spmm::num_chunks(ff), nd = spmm::num_chunks(F);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nc + nd; t += (int64_t)gridDim.x * blockDim.x) {
        if (t < nc) {
            const auto o = [&](int64_t e) { return bt::off_entry(C[e], e / F == e % F); };
            ocs[t] = spmm::chunk_sum(ff, t, o, o);
        } else {
            const auto d = [&](int64_t k) { return bt::on_entry(C[k * F + k]); };
            ocs[t] = spmm::chunk_sum(F, t - nc, d, d);
        }
    }
}

constexpr int BT_FF_CHUNKS = bt::MAX_F * bt::MAX_F / spmm::CHUNK;   // chunks of the F * F entries, at most
constexpr int BT_F_CHUNKS = bt::MAX_F / spmm::CHUNK;                // chunks of the F diagonal entries, at most
// one workgroup: the chunk sums go through LDS, one thread adds them in order
__global__ __launch_bounds__(256) void k_bt_terms(const double* __restrict__ ocs, int F, double lambd, double* __restrict__ terms) {
    __shared__ double s_cs[BT_FF_CHUNKS + BT_F_CHUNKS];
    const int64_t nc = spmm::num_chunks((int64_t)F * F), nd = spmm::num_chunks(F);   // (<= BT_FF_CHUNKS, <= BT_F_CHUNKS)
    for (int k = threadIdx.x; k < nc + nd; k += blockDim.x) s_cs[k] = ocs[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double off = 0.0, on = 0.0;
    for (int64_t k = 0; k < nc; ++k) off = off + s_cs[k];
    for (int64_t k = 0; k < nd; ++k) on = on + s_cs[nc + k];
    terms[0] = bt::loss_of(on, lambd, off);
    terms[1] = on;
    terms[2] = off;
}

// ------------------------------------------------------------------------------------------------ backward: P1 = z2 W^T, P2 = z1 W
// wp[0] = W^T and wp[1] = W, zero-padded to Fp x Fp: the B operands of the two products
__global__ __launch_bounds__(256) void k_bt_wpad(const float* __restrict__ cross, int F, int Fp, double lambd, float* __restrict__ wp) {
    const int64_t ee = (int64_t)Fp * Fp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * ee; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = e >= ee ? 1 : 0;
        const int64_t w = e - v * ee;
        const int l = (int)(w / Fp), k = (int)(w - (int64_t)l * Fp);   // element (l, k) of the operand
        float val = 0.0f;
        if (l < F && k < F) val = bt::w_of(v ? cross[(int64_t)l * F + k] : cross[(int64_t)k * F + l], k == l, lambd);
        wp[e] = val;
    }
}

struct ZR {
    const float* z[2]; const float* rp;             // z: Np x Fp each, the A operand of either product; rp: [2, Fp, Fp]
    int64_t T; int Fp, nft;
    float* P[2];                                    // Np x Fp each
};

// rlap_cca.hip's z r product: a workgroup is (product, 32-row tile); wave w owns the 32-column tiles w, w + 4, ..., NCT of them at most
template <int NCT>
__global__ __launch_bounds__(BT_THREADS) void k_bt_zr(ZR a) {
    extern __shared__ __attribute__((aligned(16))) float bt_lds[];   // 32 x Fp floats: rows l0 .. l0 + 31 of the weight
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    const int view = (int)((int64_t)blockIdx.x / a.T);               // (< 2: the grid is 2 T)
    const int64_t tile = (int64_t)blockIdx.x - view * a.T;
    const float* __restrict__ zrow = a.z[view] + (tile * bt::TILE + c) * a.Fp;   // the lane's row of z (inside the padded image)
    const float* __restrict__ rv = a.rp + (int64_t)view * a.Fp * a.Fp;
    float4 pre[4 * NCT];                                             // (4 NCT >= nft float4s a thread of a 32-row slab of the weight)
    const float4* __restrict__ rsrc = reinterpret_cast<const float4*>(rv) + threadIdx.x;
    const int row_vec = a.Fp >> 2;

    f32x16 acc[NCT];
#pragma unroll
    for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

#pragma unroll
    for (int j = 0; j < 4 * NCT; ++j) pre[j] = j < a.nft ? rsrc[j * BT_THREADS] : float4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int l0 = 0; l0 < a.Fp; l0 += bt::TILE) {
        __syncthreads();
        {
            float4* dst = reinterpret_cast<float4*>(bt_lds) + threadIdx.x;
#pragma unroll
            for (int j = 0; j < 4 * NCT; ++j)
                if (j < a.nft) dst[j * BT_THREADS] = pre[j];
        }
        __syncthreads();
        if (l0 + bt::TILE < a.Fp) {                                  // in flight while this slab is multiplied
#pragma unroll
            for (int j = 0; j < 4 * NCT; ++j)
                if (j < a.nft) pre[j] = rsrc[(l0 + bt::TILE) * row_vec + j * BT_THREADS];
        }
        const float2* __restrict__ zl = reinterpret_cast<const float2*>(zrow + l0);   // columns l0 + 2 s, l0 + 2 s + 1 of the lane's row
        const float* brow = bt_lds + h * a.Fp + c;
#pragma unroll
        for (int s = 0; s < bt::TILE / 2; ++s) {
            const float2 t = zl[s];
            const float av = h ? t.y : t.x;                          // z[row][l0 + 2 s + h]
#pragma unroll
            for (int j = 0; j < NCT; ++j) {
                const int ct = wave + 4 * j;
                if (ct < a.nft) {                                    // (wave-uniform)
                    const float bv = brow[2 * s * a.Fp + ct * bt::TILE];
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
                }
            }
        }
    }

    float* __restrict__ out = a.P[view] + tile * bt::TILE * a.Fp + c;
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
        const int ct = wave + 4 * j;
        if (ct < a.nft) {
#pragma unroll
            for (int r = 0; r < 16; ++r) out[(int64_t)bt::reg_row(r, h) * a.Fp + ct * bt::TILE] = acc[j][r];
        }
    }
}

__global__ __launch_bounds__(256) void k_bt_dh(Col a, int plain, const double* __restrict__ m, const double* __restrict__ q,
                                               float* __restrict__ ga, float* __restrict__ gb) {
    const int64_t elems = a.N * a.F;
    const double g = *a.g;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * elems; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = e >= elems ? 1 : 0;
        const int64_t w = e - v * elems, i = w / a.F;
        const int k = (int)(w - i * a.F), col = v * a.F + k;
        const double dz = bt::dz_of(g, a.P[v][i * a.Fp + k], a.N);
        (v ? gb : ga)[w] = plain ? (float)dz : bt::dh_of(dz, m[col], a.z[v][i * a.Fp + k], q[col], a.colstat[v * 2 * a.F + a.F + k], a.eps);
    }
}

// ------------------------------------------------------------------------------------------------ host
struct Bufs {
    double* cs; float *z0, *z1;
    float* partial; double* C; double* ocs;              // forward
    float* wp; float *P0, *P1; double *m, *q;            // backward
};

size_t carve_bt(Carve& C, int64_t N, int64_t F, bool backward, Bufs& B) {
    const int64_t Np = bt::padded_rows(N), Fp = bt::padded_features(F), parts = bt::num_parts(N, F);
    B = Bufs{};
    B.cs = C.take<double>(spmm::num_chunks(N) * 2 * F);
    B.z0 = C.take<float>(Np * Fp);
    B.z1 = C.take<float>(Np * Fp);
    if (!backward) {
        B.partial = C.take<float>(parts * Fp * Fp);
        B.C = C.take<double>(F * F);
        B.ocs = C.take<double>(spmm::num_chunks(F * F) + spmm::num_chunks(F));
    } else {
        B.wp = C.take<float>(2 * Fp * Fp);
        B.P0 = C.take<float>(Np * Fp);
        B.P1 = C.take<float>(Np * Fp);
        B.m = C.take<double>(2 * F);
        B.q = C.take<double>(2 * F);
    }
    return C.off + 256;
}

Col col_args(const BtArgs& g, const Bufs& B, const double* colstat) {
    Col c{};
    c.h[0] = g.a; c.h[1] = g.b; c.N = g.N; c.F = (int)g.F;
    c.z[0] = B.z0; c.z[1] = B.z1; c.P[0] = B.P0; c.P[1] = B.P1; c.Fp = bt::padded_features(g.F);
    c.colstat = colstat; c.g = g.g; c.eps = g.eps;
    c.ncols = 2 * (int)g.F; c.cs = B.cs;
    return c;
}

int launch_z(hipStream_t st, const BtArgs& g, const Bufs& B, const double* colstat) {
    const int64_t Np = bt::padded_rows(g.N);
    const int Fp = bt::padded_features(g.F);
    hipLaunchKernelGGL(k_bt_z, dim3(bt_blocks(2 * Np * Fp, 256)), dim3(256), 0, st, g.a, g.b, colstat, g.eps, g.flags & bt::NO_STANDARDIZE,
                       g.N, (int)g.F, Np, Fp, B.z0, B.z1);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

template <int NW>
int launch_cross(hipStream_t st, const Cross& m) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_cross<NW>), dim3((unsigned)(m.parts * m.groups)), dim3(BT_THREADS), 0, st, m);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

template <int NCT>
int launch_zr(hipStream_t st, const ZR& a) {
    const size_t lds = (size_t)bt::TILE * a.Fp * sizeof(float);
    if (const int rc = tile32::allow_lds(&k_bt_zr<NCT>, lds)) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_bt_zr<NCT>), dim3((unsigned)(2 * a.T)), dim3(BT_THREADS), lds, st, a);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// the instances by the header's rules; no instance (F outside [1, MAX_F], which the entry point refuses) is an error
int launch_cross_of(hipStream_t st, const Cross& m) {
    switch (bt::cross_instance(m.nft)) {
        case 1: return launch_cross<1>(st, m);
        case 2: return launch_cross<2>(st, m);
        case 4: return launch_cross<4>(st, m);
    }
    return RLAP_E_INTERNAL;
}

int launch_zr_of(hipStream_t st, const ZR& a) {
    switch (bt::zr_instance(a.nft)) {
        case 1: return launch_zr<1>(st, a);
        case 2: return launch_zr<2>(st, a);
        case 3: return launch_zr<3>(st, a);
        case 4: return launch_zr<4>(st, a);
    }
    return RLAP_E_INTERNAL;
}

}  // namespace

size_t bt_bytes(int64_t N, int64_t F) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_bt(C, N, F, false, B);
}

size_t bt_backward_bytes(int64_t N, int64_t F) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_bt(C, N, F, true, B);
}

int bt_run(hipStream_t st, void* ws, size_t ws_bytes, const BtArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_bt(C, g.N, g.F, false, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const int F = (int)g.F;
    if (!(g.flags & bt::NO_STANDARDIZE)) {   // the column statistics: the means, then the deviations, which read the means
        Col c = col_args(g, B, g.colstat);
        c.out = g.colstat;
        if (const int rc = col_sums<CS_SUM>(st, c)) return rc;
        if (const int rc = col_sums<CS_SS>(st, c)) return rc;
    }
    if (const int rc = launch_z(st, g, B, g.colstat)) return rc;
    Cross m{};
    m.z1 = B.z0; m.z2 = B.z1; m.N = g.N; m.F = F; m.Fp = bt::padded_features(g.F); m.nft = bt::feature_tiles(g.F);
    m.nst = bt::super_tiles(g.F); m.rgroups = bt::row_groups(g.F); m.groups = bt::pair_groups(g.F);
    m.parts = (int)bt::num_parts(g.N, g.F); m.partial = B.partial;
    if (const int rc = launch_cross_of(st, m)) return rc;
    const int64_t ff = (int64_t)F * F;
    hipLaunchKernelGGL(k_bt_finish, dim3(bt_blocks(ff, 256)), dim3(256), 0, st, (const float*)B.partial, m.parts, g.N, F, m.Fp, B.C, g.cross);
    hipLaunchKernelGGL(k_bt_chunks, dim3(bt_blocks(spmm::num_chunks(ff) + spmm::num_chunks(F), 256)), dim3(256), 0, st, (const double*)B.C, F, B.ocs);
    hipLaunchKernelGGL(k_bt_terms, dim3(1), dim3(256), 0, st, (const double*)B.ocs, F, g.lambd, g.terms);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int bt_backward_run(hipStream_t st, void* ws, size_t ws_bytes, const BtArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_bt(C, g.N, g.F, true, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const int F = (int)g.F;
    const int plain = g.flags & bt::NO_STANDARDIZE;
    if (const int rc = launch_z(st, g, B, g.colstat_in)) return rc;
    ZR a{};
    a.z[0] = B.z1; a.z[1] = B.z0;                                    // P1 = z2 W^T, P2 = z1 W
    a.rp = B.wp; a.T = bt::num_tiles(g.N); a.Fp = bt::padded_features(g.F); a.nft = bt::feature_tiles(g.F);
    a.P[0] = B.P0; a.P[1] = B.P1;
    hipLaunchKernelGGL(k_bt_wpad, dim3(bt_blocks(2 * (int64_t)a.Fp * a.Fp, 256)), dim3(256), 0, st, g.cross_in, F, a.Fp, g.lambd, B.wp);
    RLAP_HIPCHK(hipGetLastError());
    if (const int rc = launch_zr_of(st, a)) return rc;
    Col c = col_args(g, B, g.colstat_in);
    if (!plain) {
        c.out = B.m;
        if (const int rc = col_sums<CS_M>(st, c)) return rc;
        c.out = B.q;
        if (const int rc = col_sums<CS_Q>(st, c)) return rc;
    }
    hipLaunchKernelGGL(k_bt_dh, dim3(bt_blocks(2 * g.N * g.F, 256)), dim3(256), 0, st, c, plain, (const double*)B.m, (const double*)B.q, g.ga, g.gb);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace rlap
