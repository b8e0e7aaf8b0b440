// rlap_rowops.hip -- the fused bias, activation and dropout pass (rlap_bias_act_dropout / _backward): y = dropout(act(x
// + bias)) of an (L, N, F) tensor in one pass of 8 bytes an element, what the reference's encoders run as three torch passes behind
// every GCN and GIN layer.  The dropout coin is counter-based and drawn again in the backward pass, so no mask is kept.  Every
// value, the coin and the order of every sum are rlap_rowops.h's.  A translation unit of its own.
//
//   apply    forward.  The work items are the batch norm's (norm::item_of): lanes run along F, 16 bytes a lane where F and the
//            pointers allow, rows narrower than a wave share it; each item is cut into up to 16 row ranges while the pass has few of
//            them.  One coin word a lane and row serves its four columns.
//   bapply   backward: reads x and gy, draws the coins again, writes gx.  Where a parameter gradient is asked for, an item keeps its
//            chunk of 256 rows, the lane adds its columns' terms from 0 in row order and leaves the chunk sums in the arena.
//   finish   one workgroup per (layer, 16 columns): the chunk sums added in chunk order, streamed through LDS as the batch norm's
//            finishing kernel does it.
//   params   one thread a column goes through the layers in order: gbias, gslope per channel; one thread adds the columns in order
//            for the single slope.
// Forward is one launch, backward one, or three with parameter gradients.  No atomic touches a floating-point value, nothing
// synchronises with the host, and every element of an output is written by exactly one lane.
#include <algorithm>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "../../include/rlap_hip.h"
#include "rlap_rowops.h"
#include "rlap_rowops_api.h"
#include "rlap_spmm.h"

namespace rlap {
namespace {

constexpr int RO_WAVES = norm::GROUP_WAVES;
constexpr int RO_THREADS = RO_WAVES * 64;
constexpr int RO_DEPTH = 8;                               // rows in flight
constexpr int64_t RO_MAX_GRID = norm::MAX_GRID;           // workgroups of a launch (the kernels stride over their items)
constexpr int RO_FCOLS = 16;                              // columns of a finishing workgroup: one 128-byte line of chunk sums a row
constexpr int RO_FGROUPS = RO_THREADS / RO_FCOLS;         // rows of chunk sums its threads load side by side
constexpr int RO_FTURNS = 8;                              // loads a thread has in flight for a plane
constexpr int RO_FROWS = RO_FGROUPS * RO_FTURNS;          // chunk sums of a column staged in LDS a turn

// what the kernels share
struct Ro {
    const float* x; const float* gy; float* out;
    const float* b; const float* slope;
    float* gb; float* gs;
    int64_t L, N, F, nch;
    int flags;
    uint64_t seed; uint32_t T; double s;      // the coin: the threshold (0: no coin is drawn) and the scale of what is kept
    readout::Dispatch d;
    int split;                                // log2 of the row ranges an item is cut into (rowops::split_of)
    double* part; int planes;                 // [planes, L, nch, F] chunk sums: A, (layer norm) gweight's, C last where asked for
    double* tot;                              // [planes, L, F] their totals a layer
    // layer norm
    const float* w; float* gw;
    double eps;
    int lg;                                   // a row takes 2^lg lanes (rowops::ln_lg)
    double* rstat;                            // backward with parameter gradients: [L, N, 2] mean, rstd
};

template <int VEC> __device__ inline void ro_load(const float* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = p[0];
    } else {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
}

template <int VEC> __device__ inline void ro_store(float* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 1) p[0] = v[0];
    else *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

__device__ inline rowops::Col ro_col(const Ro& a, int64_t f) {
    rowops::Col k;
    k.b = a.b ? (double)a.b[f] : 0.0;
    k.a = (a.flags & rowops::ACT_PRELU) ? (double)a.slope[(a.flags & rowops::SLOPE_PER_CHANNEL) ? f : 0] : 0.0;
    return k;
}

// the coins of columns [f0, f0 + VEC) of row i: one word (f0 is a multiple of four on the 16-byte path)
template <int VEC> __device__ inline void ro_keep(const Ro& a, uint64_t layer, int64_t i, int64_t f0, bool (&keep)[VEC]) {
    if (a.T == 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) keep[v] = true;
        return;
    }
    const uint64_t word = rowops::coin_word(layer, i, f0 >> 2, a.F);
#pragma unroll
    for (int v = 0; v < VEC; ++v) keep[v] = rowops::keeps(rowops::coin_bits(word, f0 + v), a.T);
}

// forward: y from x
template <int VEC>
__global__ __launch_bounds__(RO_THREADS) void k_ro_apply(Ro a) {
    const int lane = threadIdx.x & 63;
    const int64_t items = norm::num_items(a.L, a.N, a.d);
    for (int64_t w = ((int64_t)blockIdx.x * RO_THREADS + threadIdx.x) >> 6; w < (items << a.split); w += (int64_t)gridDim.x * RO_WAVES) {
        norm::Item it;
        int64_t r0, r1;
        if (!norm::item_of(w >> a.split, lane, a.L, a.N, a.F, a.d, &it)) continue;
        norm::split_rows(it, a.split, w & ((1 << a.split) - 1), &r0, &r1);
        if (r0 >= r1) continue;
        rowops::Col k[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) k[v] = ro_col(a, it.f0 + v);
        const uint64_t layer = rowops::coin_layer(a.seed, it.l);
        const int64_t cnt = r1 - r0, off = (it.l * a.N + r0) * a.F + it.f0;
        const float* __restrict__ xr = a.x + off;
        float* __restrict__ yr = a.out + off;
        for (int64_t r = 0; r < cnt; r += RO_DEPTH) {
            float xv[RO_DEPTH][VEC];
#pragma unroll
            for (int u = 0; u < RO_DEPTH; ++u) ro_load<VEC>(xr + (r + u < cnt ? r + u : cnt - 1) * a.F, xv[u]);   // (a turn past the end repeats the last row)
#pragma unroll
            for (int u = 0; u < RO_DEPTH; ++u) {
                bool keep[VEC];
                ro_keep<VEC>(a, layer, r0 + r + u, it.f0, keep);
                float yv[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) yv[v] = rowops::y_of(xv[u][v], k[v], keep[v], a.s, a.flags);
                if (r + u < cnt) ro_store<VEC>(yr + (r + u) * a.F, yv);
            }
        }
    }
}

// backward: gx from x and gy, and (SUMS) the chunk sums A and (two planes) C of the item's chunk
template <int VEC, bool SUMS>
__global__ __launch_bounds__(RO_THREADS) void k_ro_bapply(Ro a) {
    const int lane = threadIdx.x & 63;
    const int64_t items = norm::num_items(a.L, a.N, a.d), plane = a.L * a.nch * a.F;
    const bool slope_sum = SUMS && a.planes == 2;
    for (int64_t w = ((int64_t)blockIdx.x * RO_THREADS + threadIdx.x) >> 6; w < (items << a.split); w += (int64_t)gridDim.x * RO_WAVES) {
        norm::Item it;
        int64_t r0, r1;
        if (!norm::item_of(w >> a.split, lane, a.L, a.N, a.F, a.d, &it)) continue;
        norm::split_rows(it, a.split, w & ((1 << a.split) - 1), &r0, &r1);   // (SUMS: the split is 0, the range the whole chunk)
        if (r0 >= r1) continue;
        rowops::Col k[VEC];
        double A[VEC], C[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) { k[v] = ro_col(a, it.f0 + v); A[v] = 0.0; C[v] = 0.0; }
        const uint64_t layer = rowops::coin_layer(a.seed, it.l);
        const int64_t cnt = r1 - r0, off = (it.l * a.N + r0) * a.F + it.f0;
        const float* __restrict__ xr = a.x + off;
        const float* __restrict__ gr = a.gy + off;
        float* __restrict__ or_ = a.out ? a.out + off : nullptr;
        for (int64_t r = 0; r < cnt; r += RO_DEPTH) {
            float xv[RO_DEPTH][VEC], gv[RO_DEPTH][VEC];
#pragma unroll
            for (int u = 0; u < RO_DEPTH; ++u) {
                const int64_t row = (r + u < cnt ? r + u : cnt - 1) * a.F;
                ro_load<VEC>(xr + row, xv[u]);
                ro_load<VEC>(gr + row, gv[u]);
            }
#pragma unroll
            for (int u = 0; u < RO_DEPTH; ++u) {
                const bool live = r + u < cnt;
                bool keep[VEC];
                ro_keep<VEC>(a, layer, r0 + r + u, it.f0, keep);
                float ov[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double g = rowops::gv_of(xv[u][v], gv[u][v], k[v], keep[v], a.s, a.flags);
                    ov[v] = (float)g;
                    if constexpr (SUMS) {
                        const double tA = spmm::accumulate(A[v], 1.0, g);
                        A[v] = live ? tA : A[v];
                        if (slope_sum) {
                            const double tC = spmm::accumulate(C[v], 1.0, rowops::slope_term(xv[u][v], gv[u][v], k[v], keep[v], a.s));
                            C[v] = live ? tC : C[v];
                        }
                    }
                }
                if (live && or_) ro_store<VEC>(or_ + (r + u) * a.F, ov);
            }
        }
        if constexpr (SUMS) {
            double* __restrict__ p = a.part + (it.l * a.nch + it.q) * a.F + it.f0;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                p[v] = A[v];
                if (slope_sum) p[plane + v] = C[v];
            }
        }
    }
}

// the totals of PLANES planes of (layers blockIdx.y, + gridDim.y ..; columns blockIdx.x * RO_FCOLS ..): 0 + the chunk sums in chunk
// order.  All threads of the workgroup load RO_FROWS rows of chunk sums (a 128-byte line each) into LDS, the next rows already in
// flight while thread kc of the first group adds the staged ones of its column -- the adds are a chain by the rule, the loads are not.
template <int PLANES>
__global__ __launch_bounds__(RO_THREADS) void k_ro_finish(Ro a) {
    __shared__ double tile[PLANES][RO_FROWS][RO_FCOLS];
    const int kc = threadIdx.x % RO_FCOLS, rg = threadIdx.x / RO_FCOLS;
    const int64_t k = (int64_t)blockIdx.x * RO_FCOLS + kc, plane = a.L * a.nch * a.F;
    const bool col = k < a.F;
    for (int64_t l = blockIdx.y; l < a.L; l += gridDim.y) {   // (the same layers for every thread of the workgroup)
        const double* __restrict__ ps = a.part + l * a.nch * a.F + (col ? k : 0);
        double v[PLANES][RO_FTURNS], total[PLANES];
        const auto load = [&](int64_t q0) {
#pragma unroll
            for (int p = 0; p < PLANES; ++p)
#pragma unroll
                for (int u = 0; u < RO_FTURNS; ++u) {
                    const int64_t q = q0 + rg + u * RO_FGROUPS;
                    v[p][u] = ps[p * plane + (q < a.nch ? q : a.nch - 1) * a.F];   // (a turn past the end repeats the last row; it is never added)
                }
        };
#pragma unroll
        for (int p = 0; p < PLANES; ++p) total[p] = 0.0;
        load(0);
        for (int64_t q0 = 0; q0 < a.nch; q0 += RO_FROWS) {   // (the same turns for every thread of the workgroup)
            __syncthreads();
#pragma unroll
            for (int p = 0; p < PLANES; ++p)
#pragma unroll
                for (int u = 0; u < RO_FTURNS; ++u) tile[p][rg + u * RO_FGROUPS][kc] = v[p][u];
            __syncthreads();
            if (q0 + RO_FROWS < a.nch) load(q0 + RO_FROWS);
            if (rg == 0 && col) {
                const int rows = a.nch - q0 < RO_FROWS ? (int)(a.nch - q0) : RO_FROWS;
                for (int r = 0; r < rows; ++r) {
#pragma unroll
                    for (int p = 0; p < PLANES; ++p) total[p] = total[p] + tile[p][r][kc];
                }
            }
        }
        if (rg == 0 && col) {
#pragma unroll
            for (int p = 0; p < PLANES; ++p) a.tot[(p * a.L + l) * a.F + k] = total[p];
        }
    }
}

// the parameter gradients: one thread a column, the layers in order; the single slope by one thread, the columns in order
__global__ __launch_bounds__(RO_THREADS) void k_ro_params(Ro a) {
    const int64_t gtid = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x;
    const bool per_channel = a.gs && (a.flags & rowops::SLOPE_PER_CHANNEL);
    const int64_t pc = (int64_t)(a.planes - 1) * a.L;   // the slope's plane is the last
    for (int64_t k = gtid; k < a.F; k += (int64_t)gridDim.x * RO_THREADS) {
        double gA = 0.0, gW = 0.0, gC = 0.0;
        for (int64_t l = 0; l < a.L; ++l) {
            gA = gA + a.tot[l * a.F + k];
            if (a.gw) gW = gW + a.tot[(a.L + l) * a.F + k];
            if (per_channel) gC = gC + a.tot[(pc + l) * a.F + k];
        }
        if (a.gb) a.gb[k] = (float)gA;
        if (a.gw) a.gw[k] = (float)gW;
        if (per_channel) a.gs[k] = (float)gC;
    }
    if (a.gs && !per_channel && gtid == 0) {
        double total = 0.0;
        for (int64_t k = 0; k < a.F; ++k) {
            double gC = 0.0;
            for (int64_t l = 0; l < a.L; ++l) gC = gC + a.tot[(pc + l) * a.F + k];
            total = total + gC;
        }
        a.gs[0] = (float)total;
    }
}

// ---- layer norm.  A row takes P = 2^lg lanes of a wave, lane t of them the columns 256 m + 4 t + v (rowops::ln_column), M steps of
// 16 bytes in registers; the 64 >> lg rows of a wave are consecutive.  The row sums are rowops::row_sum: the lane's terms in
// ascending (m, v), then the butterfly (the lanes of a narrow row run its last lg steps: the other partials are +0).  Instances of
// 1, 2 and 4 steps (up to 1024 columns); wider rows take k_ln_wide.
__device__ inline double ln_butterfly(double acc, int lg) {
    for (int off = (1 << lg) >> 1; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
    return acc;
}

// the lane's columns of one row: 0 past the row's end
template <int M, int VEC>
__device__ inline void ln_load(const float* __restrict__ row, int t, int64_t F, float (&v)[M][4]) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int64_t k0 = rowops::ln_column(t, m, 0);
        if constexpr (VEC == 4) {
            float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (k0 < F) q = *reinterpret_cast<const float4*>(row + k0);   // (F % 4 == 0: the four columns are inside together)
            v[m][0] = q.x; v[m][1] = q.y; v[m][2] = q.z; v[m][3] = q.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[m][j] = k0 + j < F ? row[k0 + j] : 0.0f;
        }
    }
}

template <int M, int VEC>
__device__ inline void ln_store(float* __restrict__ row, int t, int64_t F, const float (&v)[M][4]) {
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int64_t k0 = rowops::ln_column(t, m, 0);
        if constexpr (VEC == 4) {
            if (k0 < F) *reinterpret_cast<float4*>(row + k0) = make_float4(v[m][0], v[m][1], v[m][2], v[m][3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (k0 + j < F) row[k0 + j] = v[m][j];
        }
    }
}

__device__ inline rowops::LnCol ln_col(const Ro& a, int64_t k) {
    rowops::LnCol c;
    c.w = a.w ? (double)a.w[k] : 1.0;
    c.b = a.b ? (double)a.b[k] : 0.0;
    c.a = (a.flags & rowops::ACT_PRELU) ? (double)a.slope[(a.flags & rowops::SLOPE_PER_CHANNEL) ? k : 0] : 0.0;
    return c;
}

// mean and rstd of the row a lane group holds
template <int M>
__device__ inline rowops::Row ln_row(const Ro& a, int t, const float (&xv)[M][4]) {
    double acc = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double s = acc + (double)xv[m][j];
            acc = rowops::ln_column(t, m, j) < a.F ? s : acc;
        }
    rowops::Row r;
    r.mean = rowops::ln_mean(ln_butterfly(acc, a.lg), a.F);
    acc = 0.0;
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double s = acc + rowops::ln_square(rowops::ln_centred(xv[m][j], r.mean));
            acc = rowops::ln_column(t, m, j) < a.F ? s : acc;
        }
    r.rstd = rowops::ln_rstd(rowops::ln_mean(ln_butterfly(acc, a.lg), a.F), a.eps);
    return r;
}

// bit 4 m + j of the result: the coin of the lane's column (m, j) of row i of the layer keeps it
template <int M>
__device__ inline uint64_t ln_keep(const Ro& a, uint64_t layer, int64_t i, int t) {
    if (a.T == 0) return ~(uint64_t)0;
    uint64_t mask = 0;
#pragma unroll
    for (int m = 0; m < M; ++m) {
        const int64_t k0 = rowops::ln_column(t, m, 0);
        if (k0 < a.F) {
            const uint64_t word = rowops::coin_word(layer, i, k0 >> 2, a.F);
#pragma unroll
            for (int j = 0; j < 4; ++j) mask |= (uint64_t)(rowops::keeps(rowops::coin_bits(word, j), a.T) ? 1 : 0) << (4 * m + j);
        }
    }
    return mask;
}

// forward (BWD false): y from x.  backward: gx from x and gy, and the row's (mean, rstd) for the column sums where they follow.
// Every wave goes through its items whole; a lane group behind the last row computes on it again and stores nothing.
template <int M, int VEC, bool BWD>
__global__ __launch_bounds__(RO_THREADS) void k_ln_rows(Ro a) {
    const int lane = threadIdx.x & 63, t = lane & ((1 << a.lg) - 1), g = lane >> a.lg;
    const int64_t rows = a.L * a.N, R = 64 >> a.lg, items = (rows + R - 1) / R;
    for (int64_t w = ((int64_t)blockIdx.x * RO_THREADS + threadIdx.x) >> 6; w < items; w += (int64_t)gridDim.x * RO_WAVES) {
        const bool live = w * R + g < rows;
        const int64_t row = live ? w * R + g : rows - 1, l = row / a.N, i = row - l * a.N;
        float xv[M][4], ov[M][4];
        ln_load<M, VEC>(a.x + row * a.F, t, a.F, xv);
        const rowops::Row r = ln_row<M>(a, t, xv);
        const uint64_t keep = ln_keep<M>(a, rowops::coin_layer(a.seed, l), i, t);
        if constexpr (!BWD) {
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t k = rowops::ln_column(t, m, j);
                    ov[m][j] = k < a.F ? rowops::ln_y(xv[m][j], r, ln_col(a, k), (keep >> (4 * m + j)) & 1, a.s, a.flags) : 0.0f;
                }
        } else {
            float gv[M][4];
            ln_load<M, VEC>(a.gy + row * a.F, t, a.F, gv);
            double sg = 0.0, sgx = 0.0;
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t k = rowops::ln_column(t, m, j);
                    const bool in = k < a.F;
                    const rowops::LnCol c = ln_col(a, in ? k : 0);
                    const double gg = rowops::ln_g(rowops::ln_gv(xv[m][j], gv[m][j], r, c, (keep >> (4 * m + j)) & 1, a.s, a.flags), c);
                    const double s1 = sg + gg;
                    const double s2 = sgx + rowops::ln_gxh(gg, rowops::ln_xhat(xv[m][j], r));
                    sg = in ? s1 : sg;
                    sgx = in ? s2 : sgx;
                }
            const double mg = rowops::ln_mean(ln_butterfly(sg, a.lg), a.F), mgx = rowops::ln_mean(ln_butterfly(sgx, a.lg), a.F);
#pragma unroll
            for (int m = 0; m < M; ++m)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int64_t k = rowops::ln_column(t, m, j);
                    const rowops::LnCol c = ln_col(a, k < a.F ? k : 0);
                    const double gg = rowops::ln_g(rowops::ln_gv(xv[m][j], gv[m][j], r, c, (keep >> (4 * m + j)) & 1, a.s, a.flags), c);
                    ov[m][j] = rowops::ln_gx(gg, rowops::ln_xhat(xv[m][j], r), mg, mgx, r.rstd);
                }
            if (a.rstat && live && t == 0) { a.rstat[2 * row] = r.mean; a.rstat[2 * row + 1] = r.rstd; }
        }
        if (live && a.out) ln_store<M, VEC>(a.out + row * a.F, t, a.F, ov);
    }
}

// The same for rows of more than 1024 columns (8 or 16 steps): held in registers, the row's float64 intermediates of one pass stay
// alive for the next and the kernel spills.  Here a lane parks its own columns of x (and gy) in LDS -- it reads back only what it wrote,
// so no lane waits for another -- and every pass goes through the steps in a loop that is not unrolled.  One row a wave; the same
// values in the same order.
template <int VEC>
__device__ inline void ln_load4(const float* __restrict__ row, int64_t k0, int64_t F, float (&v)[4]) {
    if constexpr (VEC == 4) {
        float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k0 < F) q = *reinterpret_cast<const float4*>(row + k0);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = k0 + j < F ? row[k0 + j] : 0.0f;
    }
}

template <int VEC, bool BWD>
__global__ __launch_bounds__(RO_THREADS) void k_ln_wide(Ro a) {
    extern __shared__ __attribute__((aligned(16))) float ln_lds[];
    const int lane = threadIdx.x & 63, steps = rowops::ln_steps(a.F);
    float4* __restrict__ xs = reinterpret_cast<float4*>(ln_lds) + (size_t)(threadIdx.x >> 6) * steps * 64 * (BWD ? 2 : 1) + lane;
    float4* __restrict__ gs = xs + steps * 64;
    const int64_t rows = a.L * a.N;
    for (int64_t row = ((int64_t)blockIdx.x * RO_THREADS + threadIdx.x) >> 6; row < rows; row += (int64_t)gridDim.x * RO_WAVES) {
        const int64_t l = row / a.N, i = row - l * a.N;
        const uint64_t layer = rowops::coin_layer(a.seed, l);
        double acc = 0.0;
#pragma unroll 1
        for (int m = 0; m < steps; ++m) {
            const int64_t k0 = rowops::ln_column(lane, m, 0);
            float v[4];
            ln_load4<VEC>(a.x + row * a.F, k0, a.F, v);
            xs[m * 64] = make_float4(v[0], v[1], v[2], v[3]);
            if constexpr (BWD) {
                float u[4];
                ln_load4<VEC>(a.gy + row * a.F, k0, a.F, u);
                gs[m * 64] = make_float4(u[0], u[1], u[2], u[3]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double s = acc + (double)v[j];
                acc = k0 + j < a.F ? s : acc;
            }
        }
        rowops::Row r;
        r.mean = rowops::ln_mean(ln_butterfly(acc, 6), a.F);
        acc = 0.0;
#pragma unroll 1
        for (int m = 0; m < steps; ++m) {
            const int64_t k0 = rowops::ln_column(lane, m, 0);
            const float4 q = xs[m * 64];
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double s = acc + rowops::ln_square(rowops::ln_centred(v[j], r.mean));
                acc = k0 + j < a.F ? s : acc;
            }
        }
        r.rstd = rowops::ln_rstd(rowops::ln_mean(ln_butterfly(acc, 6), a.F), a.eps);
        // the coins of the lane's step m: bit j
        const auto coins = [&](int64_t k0) -> unsigned {
            if (a.T == 0 || k0 >= a.F) return 15u;
            const uint64_t word = rowops::coin_word(layer, i, k0 >> 2, a.F);
            unsigned bits = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) bits |= (rowops::keeps(rowops::coin_bits(word, j), a.T) ? 1u : 0u) << j;
            return bits;
        };
        double mg = 0.0, mgx = 0.0;
        if constexpr (BWD) {
            double sg = 0.0, sgx = 0.0;
#pragma unroll 1
            for (int m = 0; m < steps; ++m) {
                const int64_t k0 = rowops::ln_column(lane, m, 0);
                const float4 q = xs[m * 64], p = gs[m * 64];
                const float v[4] = {q.x, q.y, q.z, q.w}, u[4] = {p.x, p.y, p.z, p.w};
                const unsigned keep = coins(k0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool in = k0 + j < a.F;
                    const rowops::LnCol c = ln_col(a, in ? k0 + j : 0);
                    const double gg = rowops::ln_g(rowops::ln_gv(v[j], u[j], r, c, (keep >> j) & 1, a.s, a.flags), c);
                    const double s1 = sg + gg;
                    const double s2 = sgx + rowops::ln_gxh(gg, rowops::ln_xhat(v[j], r));
                    sg = in ? s1 : sg;
                    sgx = in ? s2 : sgx;
                }
            }
            mg = rowops::ln_mean(ln_butterfly(sg, 6), a.F);
            mgx = rowops::ln_mean(ln_butterfly(sgx, 6), a.F);
            if (a.rstat && lane == 0) { a.rstat[2 * row] = r.mean; a.rstat[2 * row + 1] = r.rstd; }
        }
        if (!a.out) continue;
#pragma unroll 1
        for (int m = 0; m < steps; ++m) {
            const int64_t k0 = rowops::ln_column(lane, m, 0);
            if (k0 >= a.F) continue;
            const float4 q = xs[m * 64];
            const float v[4] = {q.x, q.y, q.z, q.w};
            const unsigned keep = coins(k0);
            float o[4];
            if constexpr (BWD) {
                const float4 p = gs[m * 64];
                const float u[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const rowops::LnCol c = ln_col(a, k0 + j < a.F ? k0 + j : 0);
                    const double gg = rowops::ln_g(rowops::ln_gv(v[j], u[j], r, c, (keep >> j) & 1, a.s, a.flags), c);
                    o[j] = rowops::ln_gx(gg, rowops::ln_xhat(v[j], r), mg, mgx, r.rstd);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = rowops::ln_y(v[j], r, ln_col(a, k0 + j < a.F ? k0 + j : 0), (keep >> j) & 1, a.s, a.flags);
            }
            float* __restrict__ orow = a.out + row * a.F;
            if constexpr (VEC == 4) {
                *reinterpret_cast<float4*>(orow + k0) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (k0 + j < a.F) orow[k0 + j] = o[j];
            }
        }
    }
}

// backward: the chunk sums of gbias (plane 0), gweight (1) and the slope (2, where asked for), from x, gy and the rows' (mean, rstd):
// the batch norm's work items, a lane adds its columns' terms of the chunk's rows from 0 in row order
template <int VEC>
__global__ __launch_bounds__(RO_THREADS) void k_ln_bsums(Ro a) {
    const int lane = threadIdx.x & 63;
    const int64_t items = norm::num_items(a.L, a.N, a.d), plane = a.L * a.nch * a.F;
    const bool slope_sum = a.planes == 3;
    for (int64_t w = ((int64_t)blockIdx.x * RO_THREADS + threadIdx.x) >> 6; w < items; w += (int64_t)gridDim.x * RO_WAVES) {
        norm::Item it;
        if (!norm::item_of(w, lane, a.L, a.N, a.F, a.d, &it)) continue;
        rowops::LnCol k[VEC];
        double A[VEC], W[VEC], C[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) { k[v] = ln_col(a, it.f0 + v); A[v] = 0.0; W[v] = 0.0; C[v] = 0.0; }
        const uint64_t layer = rowops::coin_layer(a.seed, it.l);
        const int64_t cnt = it.r1 - it.r0, off = (it.l * a.N + it.r0) * a.F + it.f0;
        const float* __restrict__ xr = a.x + off;
        const float* __restrict__ gr = a.gy + off;
        const double* __restrict__ sr = a.rstat + 2 * (it.l * a.N + it.r0);
        for (int64_t r = 0; r < cnt; r += RO_DEPTH) {
            float xv[RO_DEPTH][VEC], gv[RO_DEPTH][VEC];
            rowops::Row rw[RO_DEPTH];
#pragma unroll
            for (int u = 0; u < RO_DEPTH; ++u) {
                const int64_t rr = r + u < cnt ? r + u : cnt - 1;
                ro_load<VEC>(xr + rr * a.F, xv[u]);
                ro_load<VEC>(gr + rr * a.F, gv[u]);
                rw[u].mean = sr[2 * rr]; rw[u].rstd = sr[2 * rr + 1];
            }
#pragma unroll
            for (int u = 0; u < RO_DEPTH; ++u) {
                const bool live = r + u < cnt;
                bool keep[VEC];
                ro_keep<VEC>(a, layer, it.r0 + r + u, it.f0, keep);
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double g = rowops::ln_gv(xv[u][v], gv[u][v], rw[u], k[v], keep[v], a.s, a.flags);
                    const double tA = spmm::accumulate(A[v], 1.0, g);
                    const double tW = spmm::accumulate(W[v], g, rowops::ln_xhat(xv[u][v], rw[u]));
                    A[v] = live ? tA : A[v];
                    W[v] = live ? tW : W[v];
                    if (slope_sum) {
                        const double tC = spmm::accumulate(C[v], 1.0, rowops::ln_slope_term(xv[u][v], gv[u][v], rw[u], k[v], keep[v], a.s));
                        C[v] = live ? tC : C[v];
                    }
                }
            }
        }
        double* __restrict__ p = a.part + (it.l * a.nch + it.q) * a.F + it.f0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            p[v] = A[v]; p[plane + v] = W[v];
            if (slope_sum) p[2 * plane + v] = C[v];
        }
    }
}

bool aligned16(const void* p, const void* q, const void* r) {
    return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(r)) & 15) == 0;
}

Ro shared_args(const RowopsArgs& g, bool aligned, bool sums) {
    Ro a{};
    a.x = g.x; a.gy = g.gy; a.out = g.out; a.b = g.bias; a.slope = g.slope; a.gb = g.gbias; a.gs = g.gslope;
    a.L = g.L; a.N = g.N; a.F = g.F; a.nch = spmm::num_chunks(g.N);
    a.flags = g.flags; a.seed = g.seed;
    a.T = rowops::threshold(g.p, g.flags);
    a.s = rowops::scale(a.T);
    a.d = norm::dispatch(g.F, aligned);
    a.split = rowops::split_of(norm::num_items(a.L, a.N, a.d), sums);
    return a;
}

unsigned apply_blocks(const Ro& a) { return capped_blocks(norm::num_items(a.L, a.N, a.d) << a.split, RO_WAVES, RO_MAX_GRID); }

void report(RowopsReport* rep, const Ro& a, int launches) {
    if (rep) { rep->vec = a.d.vec ? 1 : 0; rep->chunks = a.nch; rep->launches = launches; rep->instance = 0; }
}

int planes_of(const RowopsArgs& g) { return rowops::planes_of(g.gbias != nullptr, g.gslope != nullptr); }

}  // namespace

size_t rowops_bytes(const RowopsArgs& a, bool backward) {
    return backward ? (size_t)rowops::backward_bytes(a.L, a.N, a.F, planes_of(a)) : 0;
}

int rowops_run(hipStream_t st, void* ws, size_t ws_bytes, const RowopsArgs& g, RowopsReport* rep) {
    const Ro a = shared_args(g, aligned16(g.x, g.out, nullptr), false);
    if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_apply<4>), dim3(apply_blocks(a)), dim3(RO_THREADS), 0, st, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_apply<1>), dim3(apply_blocks(a)), dim3(RO_THREADS), 0, st, a);
    RLAP_HIPCHK(hipGetLastError());
    report(rep, a, 1);
    return RLAP_OK;
}

int rowops_backward_run(hipStream_t st, void* ws, size_t ws_bytes, const RowopsArgs& g, RowopsReport* rep) {
    if (rowops_bytes(g, true) > ws_bytes) return RLAP_E_WORKSPACE;
    const int planes = planes_of(g);
    Ro a = shared_args(g, aligned16(g.x, g.gy, g.out), planes > 0);
    a.planes = planes;
    if (planes) {
        a.part = static_cast<double*>(ws);
        a.tot = reinterpret_cast<double*>(static_cast<char*>(ws) + norm::piece(norm::part_doubles(g.L, g.N, g.F, planes)));
    }
    if (!planes && !g.out) {   // (nothing is asked for)
        report(rep, a, 0);
        return RLAP_OK;
    }
    const dim3 grid(apply_blocks(a)), block(RO_THREADS);
    if (planes) {
        if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_bapply<4, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_bapply<1, true>), grid, block, 0, st, a);
        const dim3 fgrid(grid_blocks(a.F, RO_FCOLS), (unsigned)std::min<int64_t>(a.L, RO_MAX_GRID));
        if (planes == 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_finish<2>), fgrid, block, 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_finish<1>), fgrid, block, 0, st, a);
        hipLaunchKernelGGL(k_ro_params, dim3(grid_blocks(a.F, RO_THREADS)), block, 0, st, a);
    } else {
        if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_bapply<4, false>), grid, block, 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_bapply<1, false>), grid, block, 0, st, a);
    }
    RLAP_HIPCHK(hipGetLastError());
    report(rep, a, planes ? 3 : 1);
    return RLAP_OK;
}

namespace {

template <int M, bool BWD>
void ln_launch_m(hipStream_t st, const Ro& a, unsigned blocks) {
    if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ln_rows<M, 4, BWD>), dim3(blocks), dim3(RO_THREADS), 0, st, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ln_rows<M, 1, BWD>), dim3(blocks), dim3(RO_THREADS), 0, st, a);
}

// the row kernel's instance by the 16-byte steps a lane holds (rowops::ln_instance)
template <bool BWD>
int ln_launch(hipStream_t st, const Ro& a) {
    const int64_t R = 64 >> a.lg, items = (a.L * a.N + R - 1) / R;
    const unsigned blocks = capped_blocks(items, RO_WAVES, RO_MAX_GRID);
    const int m = rowops::ln_instance(a.F);
    switch (m) {
        case 1: ln_launch_m<1, BWD>(st, a, blocks); break;
        case 2: ln_launch_m<2, BWD>(st, a, blocks); break;
        case 4: ln_launch_m<4, BWD>(st, a, blocks); break;
        default: {   // 8 or 16 steps: the row goes through LDS, one row a wave
            const size_t lds = (size_t)RO_WAVES * rowops::ln_steps(a.F) * 1024 * (BWD ? 2 : 1);
            const auto kernel = a.d.vec ? k_ln_wide<4, BWD> : k_ln_wide<1, BWD>;
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
            hipLaunchKernelGGL(kernel, dim3(blocks), dim3(RO_THREADS), lds, st, a);
        }
    }
    return m;
}

Ro ln_args(const RowopsArgs& g, bool aligned) {
    Ro a = shared_args(g, aligned, true);
    a.w = g.weight; a.gw = g.gweight; a.eps = g.eps; a.lg = rowops::ln_lg(g.F);
    return a;
}

int ln_planes_of(const RowopsArgs& g) { return rowops::ln_planes_of(g.gweight != nullptr, g.gbias != nullptr, g.gslope != nullptr); }

}  // namespace

size_t ln_bytes(const RowopsArgs& a, bool backward) {
    return backward ? (size_t)rowops::ln_backward_bytes(a.L, a.N, a.F, ln_planes_of(a)) : 0;
}

int ln_run(hipStream_t st, void* ws, size_t ws_bytes, const RowopsArgs& g, RowopsReport* rep) {
    const Ro a = ln_args(g, aligned16(g.x, g.out, nullptr));
    const int m = ln_launch<false>(st, a);
    if (m < 0) return RLAP_E_HIP;
    RLAP_HIPCHK(hipGetLastError());
    report(rep, a, 1);
    if (rep) rep->instance = m;
    return RLAP_OK;
}

int ln_backward_run(hipStream_t st, void* ws, size_t ws_bytes, const RowopsArgs& g, RowopsReport* rep) {
    if (ln_bytes(g, true) > ws_bytes) return RLAP_E_WORKSPACE;
    const int planes = ln_planes_of(g);
    Ro a = ln_args(g, aligned16(g.x, g.gy, g.out));
    a.planes = planes;
    if (!planes && !g.out) {   // (nothing is asked for)
        report(rep, a, 0);
        return RLAP_OK;
    }
    if (planes) {
        char* base = static_cast<char*>(ws);
        a.part = reinterpret_cast<double*>(base);
        a.tot = reinterpret_cast<double*>(base + norm::piece(norm::part_doubles(g.L, g.N, g.F, planes)));
        a.rstat = reinterpret_cast<double*>(base + rowops::backward_bytes(g.L, g.N, g.F, planes));
    }
    const int m = ln_launch<true>(st, a);
    if (m < 0) return RLAP_E_HIP;
    if (planes) {
        const dim3 block(RO_THREADS);
        const unsigned blocks = capped_blocks(norm::num_items(a.L, a.N, a.d), RO_WAVES, RO_MAX_GRID);
        if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ln_bsums<4>), dim3(blocks), block, 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ln_bsums<1>), dim3(blocks), block, 0, st, a);
        const dim3 fgrid(grid_blocks(a.F, RO_FCOLS), (unsigned)std::min<int64_t>(a.L, RO_MAX_GRID));
        if (planes == 3) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_finish<3>), fgrid, block, 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_finish<2>), fgrid, block, 0, st, a);
        hipLaunchKernelGGL(k_ro_params, dim3(grid_blocks(a.F, RO_THREADS)), block, 0, st, a);
    }
    RLAP_HIPCHK(hipGetLastError());
    report(rep, a, planes ? 4 : 1);
    if (rep) rep->instance = m;
    return RLAP_OK;
}

}  // namespace rlap
