// rlap_cca.hip -- the fused CCA-SSG loss, forward and backward (rlap_cca_loss / rlap_cca_loss_backward): the
// standardisation of CCA-SSG/model.py and the loss of CCA-SSG/main.py on two views' embeddings.  The Gram products z^T z are
// tall-skinny products over the node index and come from v_mfma_f32_32x32x2_f32 -- bit for bit a k-ordered float32 fmaf chain --;
// every sum has the fixed order of rlap_cca.h.  A translation unit of its own.
//
//   pre-pass   the column statistics in float64 by the chunk rule, in two passes (one thread per (chunk of 256 rows, column), lanes
//              along the columns so that the reads coalesce; then one thread per column adds the chunk sums in order); the
//              standardised copies z1, z2 in the arena, row-major, zero-padded to 32-row tiles and to a multiple of 32 columns.
//   Gram       work is (view, part of the rows, group of four super-tile pairs).  A workgroup of four waves stages 32 rows of z
//              (all Fp columns: 64 KB at F = 512) in LDS once for its waves, the next 32 rows being fetched into registers
//              meanwhile; a wave OWNS one pair (I, J), I <= J, of 64-column super tiles, that is 2 x 2 accumulator tiles (64
//              registers), and per row pair reads two A and two B operands from LDS for four MFMAs.  An operand of a step is 32 consecutive columns of two consecutive rows: lane = 32 (row & 1) + column.
//              Only the upper triangle of tiles is stored, one partial tile per part.
//   finish     the part tiles added in part order in float64, the triangle mirrored, R = delta - S / N, r = (float)R; dec1, dec2
//              by the chunk rule over R in row-major order; d_k by the chunk rule over the rows of z1 * z2; the four terms.
//   backward   z again from h and the forward's column statistics; r padded with zeros; P = z r with a 32-row tile of z as the A
//              operand (k = l; a lane reads its own row of z, eight bytes a step) and 32 rows of r staged through LDS as B, a wave
//              owning every fourth 32-column tile; then the two column sums of dz by the chunk rule and the dh pass, dz formed
//              from z and P wherever it is read.
// No float atomics, no host synchronisation, nothing allocated outside the arena.  Every address is formed from the padded sizes.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/rlap_hip.h"
#include "rlap_cca.h"
#include "rlap_cca_api.h"
#include "rlap_spmm.h"
#include "rlap_tile32_dev.h"

namespace rlap {
namespace {

using tile32::f32x16;

constexpr int CC_THREADS = 256;                 // four waves: cca::GROUP_PAIRS super-tile pairs
constexpr int64_t CC_MAX_GRID = 1 << 20;        // workgroups of a striding launch
static_assert(CC_THREADS == 64 * cca::GROUP_PAIRS, "one wave per super-tile pair");
static_assert(cca::SUPER == 2, "the Gram kernel holds 2 x 2 accumulator tiles");

inline unsigned cc_blocks(int64_t n, int per_block) { return capped_blocks(n, per_block, CC_MAX_GRID); }

// ------------------------------------------------------------------------------------------------ column sums by the chunk rule
enum { CS_SUM = 0, CS_SS = 1, CS_DOT = 2, CS_M = 3, CS_Q = 4 };

struct Col {
    const float* h[2]; int64_t N; int F;            // the inputs (CS_SUM, CS_SS)
    const float* z[2]; const float* P[2]; int Fp;   // the padded images (CS_DOT, CS_M, CS_Q)
    const double* colstat;                          // mean1 | sd1 | mean2 | sd2
    const double* g; double c4;                     // backward: the upstream gradient, (4 lambd) / N
    int ncols;                                      // F (CS_DOT) or 2 F
    double* cs;                                     // [num_chunks(N), ncols] chunk sums
    double* out;                                    // what the finish writes (see k_cca_colfinish)
};

// the term (c, x) of row i of column c of the list a mode sums
template <int MODE>
__device__ inline void cc_term(const Col& a, int64_t i, int col, double g, double* c, double* x) {
    const int v = col >= a.F ? 1 : 0, k = col - v * a.F;
    if (MODE == CS_SUM) {
        *c = 1.0; *x = (double)a.h[v][i * a.F + k];
    } else if (MODE == CS_SS) {
        const double d = cca::centred(a.h[v][i * a.F + k], a.colstat[v * 2 * a.F + k]);
        *c = d; *x = d;
    } else if (MODE == CS_DOT) {
        *c = (double)a.z[0][i * a.Fp + k]; *x = (double)a.z[1][i * a.Fp + k];
    } else {
        const double dz = cca::dz_of(g, a.z[1 - v][i * a.Fp + k], a.P[v][i * a.Fp + k], a.N, a.c4);
        if (MODE == CS_M) { *c = 1.0; *x = dz; } else { *c = dz; *x = (double)a.z[v][i * a.Fp + k]; }
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_cca_colchunks(Col a) {
    const int64_t nc = spmm::num_chunks(a.N), ncb = (a.ncols + 255) / 256;
    const double g = (MODE == CS_M || MODE == CS_Q) ? *a.g : 0.0;
    for (int64_t item = blockIdx.x; item < nc * ncb; item += gridDim.x) {
        const int64_t chunk = item / ncb;
        const int col = (int)(item - chunk * ncb) * 256 + (int)threadIdx.x;
        if (col >= a.ncols) continue;
        double s = 0.0;
        for (int64_t i = spmm::chunk_begin(chunk); i < spmm::chunk_end(a.N, chunk); ++i) {
            double c, x;
            cc_term<MODE>(a, i, col, g, &c, &x);
            s = spmm::accumulate(s, c, x);
        }
        a.cs[chunk * a.ncols + col] = s;
    }
}

// the chunk sums of a column added in order; out: CS_SUM the means and CS_SS the deviations of colstat's layout, CS_DOT d [F],
// CS_M m [2 F], CS_Q q [2 F]
template <int MODE>
__global__ __launch_bounds__(256) void k_cca_colfinish(Col a) {
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
    else if (MODE == CS_DOT) a.out[col] = total;
    else if (MODE == CS_M) a.out[col] = cca::col_m(total, a.N);
    else a.out[col] = cca::col_q(total, a.N);
}

template <int MODE>
int col_sums(hipStream_t st, const Col& a) {
    const int64_t items = spmm::num_chunks(a.N) * ((a.ncols + 255) / 256);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cca_colchunks<MODE>), dim3(cc_blocks(items, 1)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cca_colfinish<MODE>), dim3((unsigned)((a.ncols + 255) / 256)), dim3(256), 0, st, a);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// the standardised copies of both views, padded with zeros: z[v] is Np x Fp
__global__ __launch_bounds__(256) void k_cca_z(const float* __restrict__ h0, const float* __restrict__ h1, const double* __restrict__ colstat,
                                               int64_t N, int F, int64_t Np, int Fp, float* __restrict__ z0, float* __restrict__ z1) {
    const int64_t elems = Np * Fp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * elems; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = e >= elems ? 1 : 0;
        const int64_t w = e - v * elems, i = w / Fp;
        const int k = (int)(w - i * Fp);
        float val = 0.0f;
        if (i < N && k < F) val = cca::zval((v ? h1 : h0)[i * F + k], colstat[v * 2 * F + k], colstat[v * 2 * F + F + k]);
        (v ? z1 : z0)[w] = val;
    }
}

// ------------------------------------------------------------------------------------------------ the Gram product
struct Gram {
    const float* z[2];
    int64_t N; int F, Fp, nft, nst, npairs, groups, parts;
    float* partial;                                 // [2, parts, Fp, Fp]: the upper triangle of tiles is written
};

// NV >= nft: a thread stages nft float4s of a 32-row step (32 Fp / 4 = 256 nft of them), fetched into registers one step ahead
template <int NV>
__global__ __launch_bounds__(CC_THREADS) void k_cca_gram(Gram a) {
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];   // 32 x Fp floats: the rows of the step
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    int64_t b = blockIdx.x;
    const int grp = (int)(b % a.groups); b /= a.groups;
    const int part = (int)(b % a.parts);
    const int view = (int)(b / a.parts);                             // (< 2: the grid is 2 * parts * groups)
    const int q = grp * cca::GROUP_PAIRS + wave;
    const bool active = q < a.npairs;                                // (wave-uniform)
    int I, J;
    cca::pair_of(active ? q : 0, a.nst, &I, &J);
    const int ka0 = cca::tile_of(I, 0, a.nft) * cca::TILE, ka1 = cca::tile_of(I, 1, a.nft) * cca::TILE;
    const int kb0 = cca::tile_of(J, 0, a.nft) * cca::TILE, kb1 = cca::tile_of(J, 1, a.nft) * cca::TILE;
    const float* __restrict__ zv = a.z[view];
    const int64_t r0 = cca::part_begin(a.N, a.F, part), r1 = cca::part_begin(a.N, a.F, part + 1);   // (r1 <= the padded rows)
    float4 pre[NV];
    const float4* __restrict__ zsrc = reinterpret_cast<const float4*>(zv) + threadIdx.x;   // (32 rows are contiguous: 256 nft float4s)
    const int64_t row_vec = a.Fp >> 2;

    f32x16 acc00, acc01, acc10, acc11;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc00[r] = 0.0f; acc01[r] = 0.0f; acc10[r] = 0.0f; acc11[r] = 0.0f; }

#pragma unroll
    for (int j = 0; j < NV; ++j) pre[j] = j < a.nft ? zsrc[r0 * row_vec + j * CC_THREADS] : float4{0.0f, 0.0f, 0.0f, 0.0f};   // (a part is never empty)
#pragma unroll 1
    for (int64_t row = r0; row < r1; row += cca::TILE) {
        __syncthreads();   // (the previous rows have been read)
        {
            float4* dst = reinterpret_cast<float4*>(cc_lds) + threadIdx.x;
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (j < a.nft) dst[j * CC_THREADS] = pre[j];
        }
        __syncthreads();
        if (row + cca::TILE < r1) {                                  // in flight while this step is multiplied
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (j < a.nft) pre[j] = zsrc[(row + cca::TILE) * row_vec + j * CC_THREADS];
        }
        if (active) {
            const float* base = cc_lds + h * a.Fp + c;               // row (2 s + h) of the step, the lane's column of a tile
#pragma unroll 4
            for (int s = 0; s < cca::TILE / 2; ++s) {
                const float* p = base + 2 * s * a.Fp;
                const float a0 = p[ka0], a1 = p[ka1], b0 = p[kb0], b1 = p[kb1];
                acc00 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc00, 0, 0, 0);
                acc01 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc01, 0, 0, 0);
                acc10 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc10, 0, 0, 0);
                acc11 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc11, 0, 0, 0);
            }
        }
    }

    if (!active) return;
    float* __restrict__ out = a.partial + ((int64_t)view * a.parts + part) * a.Fp * a.Fp;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int ta = t >> 1, tb = t & 1;
        if (!cca::tile_stored(I, J, ta, tb, a.nft)) continue;        // (wave-uniform)
        const f32x16& acc = t == 0 ? acc00 : (t == 1 ? acc01 : (t == 2 ? acc10 : acc11));
        const int k0 = (ta ? ka1 : ka0), l0 = (tb ? kb1 : kb0);
#pragma unroll
        for (int r = 0; r < 16; ++r) out[(int64_t)(k0 + cca::reg_row(r, h)) * a.Fp + l0 + c] = acc[r];
    }
}

// S = the parts in order, the triangle mirrored, R and r
__global__ __launch_bounds__(256) void k_cca_resid(const float* __restrict__ partial, int parts, int64_t N, int F, int Fp,
                                                   double* __restrict__ R, float* __restrict__ gram) {
    const int64_t ff = (int64_t)F * F;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * ff; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = e >= ff ? 1 : 0;
        const int64_t w = e - v * ff;
        const int k = (int)(w / F), l = (int)(w - (int64_t)k * F);
        const int kk = k < l ? k : l, ll = k < l ? l : k;
        double S = 0.0;
        for (int p = 0; p < parts; ++p) S = S + (double)partial[(((int64_t)v * parts + p) * Fp + kk) * Fp + ll];
        const double r = cca::resid(S, N, k == l);
        R[e] = r;
        gram[e] = (float)r;
    }
}

// the chunk sums of R * R over the F * F entries of either view: dcs is [2, num_chunks(F F)]
__global__ __launch_bounds__(256) void k_cca_decchunks(const double* __restrict__ R, int F, double* __restrict__ dcs) {
    const int64_t ff = (int64_t)F * F, nc = spmm::num_chunks(ff);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < 2 * nc; t += (int64_t)gridDim.x * blockDim.x) {
        const int v = t >= nc ? 1 : 0;
        const double* Rv = R + v * ff;
        dcs[t] = spmm::chunk_sum(ff, t - v * nc, [&](int64_t e) { return Rv[e]; }, [&](int64_t e) { return Rv[e]; });
    }
}

constexpr int CC_FF_CHUNKS = cca::MAX_F * cca::MAX_F / spmm::CHUNK;   // chunks of the F * F entries of R, at most
// one workgroup: the chunk sums and d go through LDS, one thread adds them in order
__global__ __launch_bounds__(256) void k_cca_terms(const double* __restrict__ dcs, const double* __restrict__ d, int64_t N, int F, double lambd,
                                                   double* __restrict__ terms) {
    __shared__ double s_dcs[2 * CC_FF_CHUNKS];
    __shared__ double s_d[cca::MAX_F];
    const int64_t nc = spmm::num_chunks((int64_t)F * F);             // (<= CC_FF_CHUNKS)
    for (int k = threadIdx.x; k < 2 * nc; k += blockDim.x) s_dcs[k] = dcs[k];
    for (int k = threadIdx.x; k < F; k += blockDim.x) s_d[k] = d[k];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double dec1 = 0.0, dec2 = 0.0;
    for (int64_t k = 0; k < nc; ++k) dec1 = dec1 + s_dcs[k];
    for (int64_t k = 0; k < nc; ++k) dec2 = dec2 + s_dcs[nc + k];
    const double dsum = cca::rule_sum(F, [](int64_t) { return 1.0; }, [&](int64_t k) { return s_d[k]; });
    const double inv = cca::inv_of(dsum, N);
    terms[0] = cca::loss_of(inv, lambd, dec1, dec2);
    terms[1] = inv;
    terms[2] = dec1;
    terms[3] = dec2;
}

// ------------------------------------------------------------------------------------------------ backward: P = z r
__global__ __launch_bounds__(256) void k_cca_rpad(const float* __restrict__ gram, int F, int Fp, float* __restrict__ rp) {
    const int64_t ee = (int64_t)Fp * Fp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * ee; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = e >= ee ? 1 : 0;
        const int64_t w = e - v * ee;
        const int k = (int)(w / Fp), l = (int)(w - (int64_t)k * Fp);
        rp[e] = (k < F && l < F) ? gram[(int64_t)v * F * F + (int64_t)k * F + l] : 0.0f;
    }
}

struct ZR {
    const float* z[2]; const float* rp;             // z: Np x Fp each; rp: [2, Fp, Fp]
    int64_t T; int Fp, nft;
    float* P[2];                                    // Np x Fp each
};

// a workgroup is (view, 32-row tile); wave w owns the 32-column tiles w, w + 4, ..., NCT of them at most
template <int NCT>
__global__ __launch_bounds__(CC_THREADS) void k_cca_zr(ZR a) {
    extern __shared__ __attribute__((aligned(16))) float cc_lds[];   // 32 x Fp floats: rows l0 .. l0 + 31 of r
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, h = lane >> 5;
    const int view = (int)((int64_t)blockIdx.x / a.T);               // (< 2: the grid is 2 T)
    const int64_t tile = (int64_t)blockIdx.x - view * a.T;
    const float* __restrict__ zrow = a.z[view] + (tile * cca::TILE + c) * a.Fp;   // the lane's row of z (inside the padded image)
    const float* __restrict__ rv = a.rp + (int64_t)view * a.Fp * a.Fp;
    float4 pre[4 * NCT];                                             // (4 NCT >= nft float4s a thread of a 32-row slab of r)
    const float4* __restrict__ rsrc = reinterpret_cast<const float4*>(rv) + threadIdx.x;
    const int row_vec = a.Fp >> 2;

    f32x16 acc[NCT];
#pragma unroll
    for (int j = 0; j < NCT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;

#pragma unroll
    for (int j = 0; j < 4 * NCT; ++j) pre[j] = j < a.nft ? rsrc[j * CC_THREADS] : float4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
    for (int l0 = 0; l0 < a.Fp; l0 += cca::TILE) {
        __syncthreads();
        {
            float4* dst = reinterpret_cast<float4*>(cc_lds) + threadIdx.x;
#pragma unroll
            for (int j = 0; j < 4 * NCT; ++j)
                if (j < a.nft) dst[j * CC_THREADS] = pre[j];
        }
        __syncthreads();
        if (l0 + cca::TILE < a.Fp) {                                 // in flight while this slab is multiplied
#pragma unroll
            for (int j = 0; j < 4 * NCT; ++j)
                if (j < a.nft) pre[j] = rsrc[(l0 + cca::TILE) * row_vec + j * CC_THREADS];
        }
        const float2* __restrict__ zl = reinterpret_cast<const float2*>(zrow + l0);   // columns l0 + 2 s, l0 + 2 s + 1 of the lane's row
        const float* brow = cc_lds + h * a.Fp + c;
#pragma unroll
        for (int s = 0; s < cca::TILE / 2; ++s) {
            const float2 t = zl[s];
            const float av = h ? t.y : t.x;                          // z[row][l0 + 2 s + h]
#pragma unroll
            for (int j = 0; j < NCT; ++j) {
                const int ct = wave + 4 * j;
                if (ct < a.nft) {                                    // (wave-uniform)
                    const float bv = brow[2 * s * a.Fp + ct * cca::TILE];
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
                }
            }
        }
    }

    float* __restrict__ out = a.P[view] + tile * cca::TILE * a.Fp + c;
#pragma unroll
    for (int j = 0; j < NCT; ++j) {
        const int ct = wave + 4 * j;
        if (ct < a.nft) {
#pragma unroll
            for (int r = 0; r < 16; ++r) out[(int64_t)cca::reg_row(r, h) * a.Fp + ct * cca::TILE] = acc[j][r];
        }
    }
}

__global__ __launch_bounds__(256) void k_cca_dh(Col a, const double* __restrict__ m, const double* __restrict__ q,
                                                float* __restrict__ ga, float* __restrict__ gb) {
    const int64_t elems = a.N * a.F;
    const double g = *a.g;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < 2 * elems; e += (int64_t)gridDim.x * blockDim.x) {
        const int v = e >= elems ? 1 : 0;
        const int64_t w = e - v * elems, i = w / a.F;
        const int k = (int)(w - i * a.F), col = v * a.F + k;
        const float z = a.z[v][i * a.Fp + k];
        const double dz = cca::dz_of(g, a.z[1 - v][i * a.Fp + k], a.P[v][i * a.Fp + k], a.N, a.c4);
        (v ? gb : ga)[w] = cca::dh_of(dz, m[col], z, q[col], a.colstat[v * 2 * a.F + a.F + k]);
    }
}

// ------------------------------------------------------------------------------------------------ host
struct Bufs {
    double* cs; float *z0, *z1;
    double* d; float* partial; double* R; double* dcs;   // forward
    float* rp; float *P0, *P1; double *m, *q;            // backward
};

size_t carve_cca(Carve& C, int64_t N, int64_t F, bool backward, Bufs& B) {
    const int64_t Np = cca::padded_rows(N), Fp = cca::padded_features(F), parts = cca::num_parts(N, F);
    B = Bufs{};
    B.cs = C.take<double>(spmm::num_chunks(N) * 2 * F);
    B.z0 = C.take<float>(Np * Fp);
    B.z1 = C.take<float>(Np * Fp);
    if (!backward) {
        B.d = C.take<double>(F);
        B.partial = C.take<float>(2 * parts * Fp * Fp);
        B.R = C.take<double>(2 * F * F);
        B.dcs = C.take<double>(2 * spmm::num_chunks(F * F));
    } else {
        B.rp = C.take<float>(2 * Fp * Fp);
        B.P0 = C.take<float>(Np * Fp);
        B.P1 = C.take<float>(Np * Fp);
        B.m = C.take<double>(2 * F);
        B.q = C.take<double>(2 * F);
    }
    return C.off + 256;
}

Col col_args(const CcaArgs& g, const Bufs& B, const double* colstat) {
    Col c{};
    c.h[0] = g.a; c.h[1] = g.b; c.N = g.N; c.F = (int)g.F;
    c.z[0] = B.z0; c.z[1] = B.z1; c.P[0] = B.P0; c.P[1] = B.P1; c.Fp = cca::padded_features(g.F);
    c.colstat = colstat; c.g = g.g; c.c4 = cca::coef4(g.lambd, g.N);
    c.ncols = 2 * (int)g.F; c.cs = B.cs;
    return c;
}

int launch_z(hipStream_t st, const CcaArgs& g, const Bufs& B, const double* colstat) {
    const int64_t Np = cca::padded_rows(g.N);
    const int Fp = cca::padded_features(g.F);
    hipLaunchKernelGGL(k_cca_z, dim3(cc_blocks(2 * Np * Fp, 256)), dim3(256), 0, st, g.a, g.b, colstat, g.N, (int)g.F, Np, Fp, B.z0, B.z1);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

template <int NV>
int launch_gram(hipStream_t st, const Gram& m) {
    const size_t lds = (size_t)cca::TILE * m.Fp * sizeof(float);
    if (const int rc = tile32::allow_lds(&k_cca_gram<NV>, lds)) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cca_gram<NV>), dim3((unsigned)(2 * m.parts * m.groups)), dim3(CC_THREADS), lds, st, m);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

template <int NCT>
int launch_zr(hipStream_t st, const ZR& a) {
    const size_t lds = (size_t)cca::TILE * a.Fp * sizeof(float);
    if (const int rc = tile32::allow_lds(&k_cca_zr<NCT>, lds)) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_cca_zr<NCT>), dim3((unsigned)(2 * a.T)), dim3(CC_THREADS), lds, st, a);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// the instances by the header's rules; no instance (F outside [1, MAX_F], which the entry point refuses) is an error
int launch_gram_of(hipStream_t st, const Gram& m) {
    return tile32::ladder_launch(m.nft, [&](auto nv) { return launch_gram<decltype(nv)::value>(st, m); });
}

int launch_zr_of(hipStream_t st, const ZR& a) {
    switch (cca::zr_instance(a.nft)) {
        case 1: return launch_zr<1>(st, a);
        case 2: return launch_zr<2>(st, a);
        case 3: return launch_zr<3>(st, a);
        case 4: return launch_zr<4>(st, a);
    }
    return RLAP_E_INTERNAL;
}

}  // namespace

size_t cca_bytes(int64_t N, int64_t F) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_cca(C, N, F, false, B);
}

size_t cca_backward_bytes(int64_t N, int64_t F) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_cca(C, N, F, true, B);
}

int cca_run(hipStream_t st, void* ws, size_t ws_bytes, const CcaArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_cca(C, g.N, g.F, false, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const int F = (int)g.F;
    // the column statistics: the means, then the deviations, which read the means
    Col c = col_args(g, B, g.colstat);
    c.out = g.colstat;
    if (const int rc = col_sums<CS_SUM>(st, c)) return rc;
    if (const int rc = col_sums<CS_SS>(st, c)) return rc;
    if (const int rc = launch_z(st, g, B, g.colstat)) return rc;
    c.ncols = F; c.out = B.d;
    if (const int rc = col_sums<CS_DOT>(st, c)) return rc;
    // the Gram products of both views
    Gram m{};
    m.z[0] = B.z0; m.z[1] = B.z1; m.N = g.N; m.F = F; m.Fp = cca::padded_features(g.F); m.nft = cca::feature_tiles(g.F);
    m.nst = cca::super_tiles(g.F); m.npairs = cca::super_pairs(g.F); m.groups = cca::pair_groups(g.F);
    m.parts = (int)cca::num_parts(g.N, g.F); m.partial = B.partial;
    if (const int rc = launch_gram_of(st, m)) return rc;
    hipLaunchKernelGGL(k_cca_resid, dim3(cc_blocks(2 * (int64_t)F * F, 256)), dim3(256), 0, st, (const float*)B.partial, m.parts, g.N, F, m.Fp, B.R, g.gram);
    hipLaunchKernelGGL(k_cca_decchunks, dim3(cc_blocks(2 * spmm::num_chunks((int64_t)F * F), 256)), dim3(256), 0, st, (const double*)B.R, F, B.dcs);
    hipLaunchKernelGGL(k_cca_terms, dim3(1), dim3(256), 0, st, (const double*)B.dcs, (const double*)B.d, g.N, F, g.lambd, g.terms);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int cca_backward_run(hipStream_t st, void* ws, size_t ws_bytes, const CcaArgs& g) {
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_cca(C, g.N, g.F, true, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const int F = (int)g.F;
    if (const int rc = launch_z(st, g, B, g.colstat_in)) return rc;
    ZR a{};
    a.z[0] = B.z0; a.z[1] = B.z1; a.rp = B.rp; a.T = cca::num_tiles(g.N); a.Fp = cca::padded_features(g.F); a.nft = cca::feature_tiles(g.F);
    a.P[0] = B.P0; a.P[1] = B.P1;
    hipLaunchKernelGGL(k_cca_rpad, dim3(cc_blocks(2 * (int64_t)a.Fp * a.Fp, 256)), dim3(256), 0, st, g.gram_in, F, a.Fp, B.rp);
    RLAP_HIPCHK(hipGetLastError());
    if (const int rc = launch_zr_of(st, a)) return rc;
    Col c = col_args(g, B, g.colstat_in);
    c.out = B.m;
    if (const int rc = col_sums<CS_M>(st, c)) return rc;
    c.out = B.q;
    if (const int rc = col_sums<CS_Q>(st, c)) return rc;
    hipLaunchKernelGGL(k_cca_dh, dim3(cc_blocks(2 * g.N * g.F, 256)), dim3(256), 0, st, c, (const double*)B.m, (const double*)B.q, g.ga, g.gb);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace rlap
