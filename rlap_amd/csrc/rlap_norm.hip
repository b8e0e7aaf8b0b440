// rlap_norm.hip -- per-view batch norm with fused activations (rlap_batch_norm / _backward): every layer of an (L, N, F)
// tensor is normalised with its own column statistics, a ReLU in front and a ReLU or PReLU behind fused in, the running buffers
// updated once a layer in layer order -- what the reference's encoders do by one BatchNorm1d call a view.  Every value and the order
// of every sum are rlap_norm.h's.  A translation unit of its own.
//
//   sums     one work item per (layer, group of chunks, column tile), norm::item_of: lanes run along F, 16 bytes a lane where F and the
//            pointers allow; a lane adds its columns of the chunk's 256 rows from 0 in row order (spmm::accumulate), NM_DEPTH rows of
//            x in flight before the dependent adds, and leaves the chunk sums in the arena.  Rows narrower than a wave share it with
//            the rows of the next chunks, so that every lane has a column.
//   finish   one workgroup per (layer, 16 columns): the chunk sums added in chunk order -- all its threads stream them through LDS, one
//            thread a column adds them --, then the statistics and `stat` (forward) or A / N and B / N (backward).
//   apply    the same work items, each cut into up to 16 row ranges while the pass has few of them (norm::apply_split: this pass has
//            no order to keep): reads x (and gy), forms u, xh and v again, writes y (or gx).  In front of it one thread a column
//            goes through the layers in order: the running buffers (forward), the parameter gradients (backward).
// Training forward and backward are these three launches each; evaluation mode is the apply pass alone, with the sums only where a
// parameter gradient is asked for.  No atomic touches a
// floating-point value, nothing synchronises with the host, and every element of an output is written by exactly one lane.
#include <algorithm>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "../../include/rlap_hip.h"
#include "rlap_norm.h"
#include "rlap_norm_api.h"
#include "rlap_spmm.h"

namespace rlap {
namespace {

constexpr int NM_WAVES = norm::GROUP_WAVES;
constexpr int NM_THREADS = NM_WAVES * 64;
constexpr int NM_DEPTH = 16;                              // rows in flight (forward)
constexpr int NM_BDEPTH = 8;                              // rows of x and of gy in flight (backward)
constexpr int64_t NM_MAX_GRID = norm::MAX_GRID;           // workgroups of a launch (the kernels stride over their items)
constexpr int NM_FCOLS = 16;                              // columns of a finishing workgroup: one 128-byte line of chunk sums a row
constexpr int NM_FGROUPS = NM_THREADS / NM_FCOLS;         // rows of chunk sums its threads load side by side
constexpr int NM_FTURNS = 8;                              // loads a thread has in flight for a plane
constexpr int NM_FROWS = NM_FGROUPS * NM_FTURNS;          // chunk sums of a column staged in LDS a turn

// what the kernels share
struct Nm {
    const float* x; const float* gy; float* out;
    const float* w; const float* b; const float* slope;
    const float* rmean; const float* rvar;    // evaluation mode
    float* upd_mean; float* upd_var;
    double* stat;
    float* gw; float* gb; float* gs;
    int64_t L, N, F, nch;
    int flags;
    double eps, momentum;
    readout::Dispatch d;
    int split;                                // log2 of the row ranges an item of the apply passes is cut into (norm::apply_split)
    double* part; int sums;                   // [sums, L, nch, F] chunk sums
    double* mv;                               // forward [2, L, F] mean, unbiased variance; backward [2, L, F] A / N, B / N
    double* tot;                              // backward [3, L, F] A, B, C
};

template <int VEC> __device__ inline void nm_load(const float* __restrict__ p, float (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = p[0];
    } else {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
}

template <int VEC> __device__ inline void nm_store(float* __restrict__ p, const float (&v)[VEC]) {
    if constexpr (VEC == 1) p[0] = v[0];
    else *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// what column f of layer l shares (rlap_norm.h: Col)
__device__ inline norm::Col nm_col(const Nm& a, int64_t l, int64_t f) {
    norm::Col k;
    if (a.flags & norm::EVAL) {
        k.c = (double)a.rmean[f]; k.m = 0.0; k.rstd = norm::col_rstd((double)a.rvar[f], a.eps);
    } else {
        const double* __restrict__ s = a.stat + l * 3 * a.F;
        k.c = s[f]; k.m = s[a.F + f]; k.rstd = s[2 * a.F + f];
    }
    k.w = a.w ? (double)a.w[f] : 1.0;
    k.b = a.b ? (double)a.b[f] : 0.0;
    k.a = (a.flags & norm::POST_PRELU) ? (double)a.slope[(a.flags & norm::SLOPE_PER_CHANNEL) ? f : 0] : 0.0;
    return k;
}

// forward: the chunk sums s1 and s2 of d = u - c
template <int VEC>
__global__ __launch_bounds__(NM_THREADS) void k_nm_sums(Nm a) {
    const int lane = threadIdx.x & 63;
    const int64_t items = norm::num_items(a.L, a.N, a.d), plane = a.L * a.nch * a.F;
    for (int64_t w = ((int64_t)blockIdx.x * NM_THREADS + threadIdx.x) >> 6; w < items; w += (int64_t)gridDim.x * NM_WAVES) {
        norm::Item it;
        if (!norm::item_of(w, lane, a.L, a.N, a.F, a.d, &it)) continue;
        const float* __restrict__ xl = a.x + it.l * a.N * a.F + it.f0;
        float x0[VEC];
        nm_load<VEC>(xl, x0);
        double c[VEC], s1[VEC], s2[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) { c[v] = norm::pre(x0[v], a.flags); s1[v] = 0.0; s2[v] = 0.0; }
        const int64_t cnt = it.r1 - it.r0;
        const float* __restrict__ xr = xl + it.r0 * a.F;
        for (int64_t r = 0; r < cnt; r += NM_DEPTH) {
            float xv[NM_DEPTH][VEC];
#pragma unroll
            for (int u = 0; u < NM_DEPTH; ++u) nm_load<VEC>(xr + (r + u < cnt ? r + u : cnt - 1) * a.F, xv[u]);   // (a turn past the end repeats the last row)
#pragma unroll
            for (int u = 0; u < NM_DEPTH; ++u) {
                const bool live = r + u < cnt;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double d = norm::pre(xv[u][v], a.flags) - c[v];
                    const double t1 = spmm::accumulate(s1[v], 1.0, d);
                    const double t2 = spmm::accumulate(s2[v], d, d);
                    s1[v] = live ? t1 : s1[v];
                    s2[v] = live ? t2 : s2[v];
                }
            }
        }
        double* __restrict__ p = a.part + (it.l * a.nch + it.q) * a.F + it.f0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) { p[v] = s1[v]; p[plane + v] = s2[v]; }
    }
}

// 0 + the chunk sums of PLANES planes of (layer l, columns k0 ..), in chunk order, by one workgroup: all its threads load NM_FROWS
// rows of chunk sums (a 128-byte line each) into LDS, the next rows already in flight while thread kc of the first group adds the
// staged ones of column k0 + kc -- the adds are a chain by the rule, the loads are not.  total[] is that thread's.
template <int PLANES>
__device__ inline void nm_totals(const Nm& a, int64_t l, int64_t k0, double (&total)[PLANES]) {
    __shared__ double tile[PLANES][NM_FROWS][NM_FCOLS];
    const int kc = threadIdx.x % NM_FCOLS, rg = threadIdx.x / NM_FCOLS;
    const int64_t k = k0 + kc, plane = a.L * a.nch * a.F;
    const bool col = k < a.F;
    const double* __restrict__ ps = a.part + l * a.nch * a.F + (col ? k : 0);
    double v[PLANES][NM_FTURNS];
    const auto load = [&](int64_t q0) {
#pragma unroll
        for (int p = 0; p < PLANES; ++p)
#pragma unroll
            for (int u = 0; u < NM_FTURNS; ++u) {
                const int64_t q = q0 + rg + u * NM_FGROUPS;
                v[p][u] = ps[p * plane + (q < a.nch ? q : a.nch - 1) * a.F];   // (a turn past the end repeats the last row; it is never added)
            }
    };
#pragma unroll
    for (int p = 0; p < PLANES; ++p) total[p] = 0.0;
    load(0);
    for (int64_t q0 = 0; q0 < a.nch; q0 += NM_FROWS) {   // (the same turns for every thread of the workgroup)
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PLANES; ++p)
#pragma unroll
            for (int u = 0; u < NM_FTURNS; ++u) tile[p][rg + u * NM_FGROUPS][kc] = v[p][u];
        __syncthreads();
        if (q0 + NM_FROWS < a.nch) load(q0 + NM_FROWS);
        if (rg == 0 && col) {
            const int rows = a.nch - q0 < NM_FROWS ? (int)(a.nch - q0) : NM_FROWS;
            for (int r = 0; r < rows; ++r) {
#pragma unroll
                for (int p = 0; p < PLANES; ++p) total[p] = total[p] + tile[p][r][kc];
            }
        }
    }
}

// forward: the statistics of (layers blockIdx.y, + gridDim.y ..; columns blockIdx.x * NM_FCOLS ..): `stat`, and the mean and the unbiased variance for
// the running buffers, which the apply pass updates
__global__ __launch_bounds__(NM_THREADS) void k_nm_stats(Nm a) {
    const int64_t k = (int64_t)blockIdx.x * NM_FCOLS + threadIdx.x;
    for (int64_t l = blockIdx.y; l < a.L; l += gridDim.y) {   // (the same layers for every thread of the workgroup)
        double total[2];
        nm_totals<2>(a, l, (int64_t)blockIdx.x * NM_FCOLS, total);
        if (threadIdx.x >= NM_FCOLS || k >= a.F) continue;
        const double c = norm::pre(a.x[l * a.N * a.F + k], a.flags);
        const double m = norm::col_m(total[0], a.N);
        const double var = norm::col_var(total[1], m, a.N);
        double* __restrict__ s = a.stat + l * 3 * a.F;
        s[k] = c; s[a.F + k] = m; s[2 * a.F + k] = norm::col_rstd(var, a.eps);
        a.mv[l * a.F + k] = norm::col_mean(c, m);
        a.mv[(a.L + l) * a.F + k] = norm::unbiased(var, a.N);
    }
}

// forward: y from x and the columns' constants
template <int VEC>
__global__ __launch_bounds__(NM_THREADS) void k_nm_apply(Nm a) {
    const int lane = threadIdx.x & 63;
    const int64_t items = norm::num_items(a.L, a.N, a.d);
    if (a.upd_mean || a.upd_var) {   // the running buffers, one thread a column, the layers in order
        for (int64_t k = (int64_t)blockIdx.x * NM_THREADS + threadIdx.x; k < a.F; k += (int64_t)gridDim.x * NM_THREADS) {
            float rm = a.upd_mean ? a.upd_mean[k] : 0.0f, rv = a.upd_var ? a.upd_var[k] : 0.0f;
            for (int64_t l = 0; l < a.L; ++l) {
                rm = norm::running(rm, a.momentum, a.mv[l * a.F + k]);
                rv = norm::running(rv, a.momentum, a.mv[(a.L + l) * a.F + k]);
            }
            if (a.upd_mean) a.upd_mean[k] = rm;
            if (a.upd_var) a.upd_var[k] = rv;
        }
    }
    for (int64_t w = ((int64_t)blockIdx.x * NM_THREADS + threadIdx.x) >> 6; w < (items << a.split); w += (int64_t)gridDim.x * NM_WAVES) {
        norm::Item it;
        int64_t r0, r1;
        if (!norm::item_of(w >> a.split, lane, a.L, a.N, a.F, a.d, &it)) continue;
        norm::split_rows(it, a.split, w & ((1 << a.split) - 1), &r0, &r1);
        if (r0 >= r1) continue;
        norm::Col k[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) k[v] = nm_col(a, it.l, it.f0 + v);
        const int64_t cnt = r1 - r0, off = (it.l * a.N + r0) * a.F + it.f0;
        const float* __restrict__ xr = a.x + off;
        float* __restrict__ yr = a.out + off;
        for (int64_t r = 0; r < cnt; r += NM_DEPTH) {
            float xv[NM_DEPTH][VEC];
#pragma unroll
            for (int u = 0; u < NM_DEPTH; ++u) nm_load<VEC>(xr + (r + u < cnt ? r + u : cnt - 1) * a.F, xv[u]);
#pragma unroll
            for (int u = 0; u < NM_DEPTH; ++u) {
                float yv[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) yv[v] = norm::y_of(xv[u][v], k[v], a.flags);
                if (r + u < cnt) nm_store<VEC>(yr + (r + u) * a.F, yv);
            }
        }
    }
}

// backward: the chunk sums A, B and (PReLU) C
template <int VEC>
__global__ __launch_bounds__(NM_THREADS) void k_nm_bsums(Nm a) {
    const int lane = threadIdx.x & 63;
    const int64_t items = norm::num_items(a.L, a.N, a.d), plane = a.L * a.nch * a.F;
    const bool prelu = (a.flags & norm::POST_PRELU) != 0;
    for (int64_t w = ((int64_t)blockIdx.x * NM_THREADS + threadIdx.x) >> 6; w < items; w += (int64_t)gridDim.x * NM_WAVES) {
        norm::Item it;
        if (!norm::item_of(w, lane, a.L, a.N, a.F, a.d, &it)) continue;
        norm::Col k[VEC];
        double A[VEC], B[VEC], C[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) { k[v] = nm_col(a, it.l, it.f0 + v); A[v] = 0.0; B[v] = 0.0; C[v] = 0.0; }
        const int64_t cnt = it.r1 - it.r0, off = (it.l * a.N + it.r0) * a.F + it.f0;
        const float* __restrict__ xr = a.x + off;
        const float* __restrict__ gr = a.gy + off;
        for (int64_t r = 0; r < cnt; r += NM_BDEPTH) {
            float xv[NM_BDEPTH][VEC], gv[NM_BDEPTH][VEC];
#pragma unroll
            for (int u = 0; u < NM_BDEPTH; ++u) {
                const int64_t row = (r + u < cnt ? r + u : cnt - 1) * a.F;
                nm_load<VEC>(xr + row, xv[u]);
                nm_load<VEC>(gr + row, gv[u]);
            }
#pragma unroll
            for (int u = 0; u < NM_BDEPTH; ++u) {
                const bool live = r + u < cnt;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double xh = norm::xhat(norm::pre(xv[u][v], a.flags), k[v], a.flags);
                    const double val = norm::affine(xh, k[v]);
                    const double g = norm::gv_of(gv[u][v], val, k[v], a.flags);
                    const double tA = spmm::accumulate(A[v], 1.0, g);
                    const double tB = spmm::accumulate(B[v], g, xh);
                    A[v] = live ? tA : A[v];
                    B[v] = live ? tB : B[v];
                    if (prelu) {
                        const double tC = spmm::accumulate(C[v], 1.0, norm::slope_term(gv[u][v], val));
                        C[v] = live ? tC : C[v];
                    }
                }
            }
        }
        double* __restrict__ p = a.part + (it.l * a.nch + it.q) * a.F + it.f0;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            p[v] = A[v]; p[plane + v] = B[v];
            if (prelu) p[2 * plane + v] = C[v];
        }
    }
}

// backward: the totals A, B and (PLANES == 3) C of (layers blockIdx.y, + gridDim.y ..; columns blockIdx.x * NM_FCOLS ..), and A / N and B / N
template <int PLANES>
__global__ __launch_bounds__(NM_THREADS) void k_nm_bfinish(Nm a) {
    const int64_t k = (int64_t)blockIdx.x * NM_FCOLS + threadIdx.x;
    for (int64_t l = blockIdx.y; l < a.L; l += gridDim.y) {   // (the same layers for every thread of the workgroup)
        double total[PLANES];
        nm_totals<PLANES>(a, l, (int64_t)blockIdx.x * NM_FCOLS, total);
        if (threadIdx.x >= NM_FCOLS || k >= a.F) continue;
        a.mv[l * a.F + k] = norm::col_m(total[0], a.N);
        a.mv[(a.L + l) * a.F + k] = norm::col_m(total[1], a.N);
#pragma unroll
        for (int p = 0; p < PLANES; ++p) a.tot[(p * a.L + l) * a.F + k] = total[p];
    }
}

// backward: gx from x, gy and the columns' constants
template <int VEC>
__global__ __launch_bounds__(NM_THREADS) void k_nm_bapply(Nm a) {
    const int lane = threadIdx.x & 63;
    const int64_t items = norm::num_items(a.L, a.N, a.d);
    const bool eval = (a.flags & norm::EVAL) != 0, prelu = (a.flags & norm::POST_PRELU) != 0;
    const int64_t gtid = (int64_t)blockIdx.x * NM_THREADS + threadIdx.x;
    if (a.gw || a.gb || a.gs) {   // the parameter gradients, one thread a column, the layers in order
        const bool per_channel = prelu && a.gs && (a.flags & norm::SLOPE_PER_CHANNEL);
        for (int64_t k = gtid; k < a.F; k += (int64_t)gridDim.x * NM_THREADS) {
            double gA = 0.0, gB = 0.0, gC = 0.0;
            for (int64_t l = 0; l < a.L; ++l) {
                gA = gA + a.tot[l * a.F + k];
                gB = gB + a.tot[(a.L + l) * a.F + k];
                if (per_channel) gC = gC + a.tot[(2 * a.L + l) * a.F + k];
            }
            if (a.gb) a.gb[k] = (float)gA;
            if (a.gw) a.gw[k] = (float)gB;
            if (per_channel) a.gs[k] = (float)gC;
        }
        if (prelu && a.gs && !per_channel && gtid == 0) {   // the single slope: the columns' sums in column order
            double total = 0.0;
            for (int64_t k = 0; k < a.F; ++k) {
                double gC = 0.0;
                for (int64_t l = 0; l < a.L; ++l) gC = gC + a.tot[(2 * a.L + l) * a.F + k];
                total = total + gC;
            }
            a.gs[0] = (float)total;
        }
    }
    if (!a.out) return;
    for (int64_t w = gtid >> 6; w < (items << a.split); w += (int64_t)gridDim.x * NM_WAVES) {
        norm::Item it;
        int64_t r0, r1;
        if (!norm::item_of(w >> a.split, lane, a.L, a.N, a.F, a.d, &it)) continue;
        norm::split_rows(it, a.split, w & ((1 << a.split) - 1), &r0, &r1);
        if (r0 >= r1) continue;
        norm::Col k[VEC];
        double An[VEC], Bn[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            k[v] = nm_col(a, it.l, it.f0 + v);
            An[v] = eval ? 0.0 : a.mv[it.l * a.F + it.f0 + v];
            Bn[v] = eval ? 0.0 : a.mv[(a.L + it.l) * a.F + it.f0 + v];
        }
        const int64_t cnt = r1 - r0, off = (it.l * a.N + r0) * a.F + it.f0;
        const float* __restrict__ xr = a.x + off;
        const float* __restrict__ gr = a.gy + off;
        float* __restrict__ or_ = a.out + off;
        for (int64_t r = 0; r < cnt; r += NM_BDEPTH) {
            float xv[NM_BDEPTH][VEC], gv[NM_BDEPTH][VEC];
#pragma unroll
            for (int u = 0; u < NM_BDEPTH; ++u) {
                const int64_t row = (r + u < cnt ? r + u : cnt - 1) * a.F;
                nm_load<VEC>(xr + row, xv[u]);
                nm_load<VEC>(gr + row, gv[u]);
            }
#pragma unroll
            for (int u = 0; u < NM_BDEPTH; ++u) {
                float ov[VEC];
#pragma unroll
                for (int v = 0; v < VEC; ++v) ov[v] = norm::gx_of(xv[u][v], gv[u][v], k[v], An[v], Bn[v], a.flags);
                if (r + u < cnt) nm_store<VEC>(or_ + (r + u) * a.F, ov);
            }
        }
    }
}

bool aligned16(const void* p, const void* q, const void* r) {
    return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(r)) & 15) == 0;
}

Nm shared_args(const NormArgs& g, bool aligned) {
    Nm a{};
    a.x = g.x; a.gy = g.gy; a.out = g.out; a.w = g.weight; a.b = g.bias; a.slope = g.slope;
    a.rmean = g.running_mean; a.rvar = g.running_var; a.upd_mean = g.upd_mean; a.upd_var = g.upd_var;
    a.stat = g.stat; a.gw = g.gweight; a.gb = g.gbias; a.gs = g.gslope;
    a.L = g.L; a.N = g.N; a.F = g.F; a.nch = spmm::num_chunks(g.N);
    a.flags = g.flags; a.eps = g.eps; a.momentum = g.momentum;
    a.d = norm::dispatch(g.F, aligned);
    a.split = norm::apply_split(norm::num_items(a.L, a.N, a.d));
    return a;
}

unsigned item_blocks(const Nm& a) { return capped_blocks(norm::num_items(a.L, a.N, a.d), NM_WAVES, NM_MAX_GRID); }
unsigned apply_blocks(const Nm& a) { return capped_blocks(norm::num_items(a.L, a.N, a.d) << a.split, NM_WAVES, NM_MAX_GRID); }
dim3 finish_blocks(const Nm& a) { return dim3(grid_blocks(a.F, NM_FCOLS), (unsigned)std::min<int64_t>(a.L, NM_MAX_GRID)); }

void report(NormReport* rep, const Nm& a, int launches) {
    if (rep) { rep->vec = a.d.vec ? 1 : 0; rep->chunks = a.nch; rep->launches = launches; }
}

}  // namespace

size_t norm_bytes(const NormArgs& a, bool backward) {
    return (size_t)(backward ? norm::backward_bytes(a.L, a.N, a.F, a.flags) : norm::forward_bytes(a.L, a.N, a.F, a.flags));
}

int norm_run(hipStream_t st, void* ws, size_t ws_bytes, const NormArgs& g, NormReport* rep) {
    if (norm_bytes(g, false) > ws_bytes) return RLAP_E_WORKSPACE;
    Nm a = shared_args(g, aligned16(g.x, g.out, nullptr));
    a.part = static_cast<double*>(ws); a.sums = 2;
    a.mv = reinterpret_cast<double*>(static_cast<char*>(ws) + norm::piece(norm::part_doubles(g.L, g.N, g.F, 2)));
    int launches = 0;
    if (!(g.flags & norm::EVAL)) {
        if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_sums<4>), dim3(item_blocks(a)), dim3(NM_THREADS), 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_sums<1>), dim3(item_blocks(a)), dim3(NM_THREADS), 0, st, a);
        hipLaunchKernelGGL(k_nm_stats, finish_blocks(a), dim3(NM_THREADS), 0, st, a);
        launches += 2;
    }
    if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_apply<4>), dim3(apply_blocks(a)), dim3(NM_THREADS), 0, st, a);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_apply<1>), dim3(apply_blocks(a)), dim3(NM_THREADS), 0, st, a);
    RLAP_HIPCHK(hipGetLastError());
    report(rep, a, launches + 1);
    return RLAP_OK;
}

int norm_backward_run(hipStream_t st, void* ws, size_t ws_bytes, const NormArgs& g, NormReport* rep) {
    if (norm_bytes(g, true) > ws_bytes) return RLAP_E_WORKSPACE;
    Nm a = shared_args(g, aligned16(g.x, g.gy, g.out));
    a.sums = norm::backward_sums(g.flags);
    char* base = static_cast<char*>(ws);
    a.part = reinterpret_cast<double*>(base);
    a.mv = reinterpret_cast<double*>(base + norm::piece(norm::part_doubles(g.L, g.N, g.F, a.sums)));
    a.tot = reinterpret_cast<double*>(base + norm::piece(norm::part_doubles(g.L, g.N, g.F, a.sums)) + norm::piece(2 * g.L * g.F));
    const bool params = g.gweight || g.gbias || g.gslope;
    int launches = 0;
    if (!(g.flags & norm::EVAL) || params) {   // (evaluation mode: the sums serve the parameter gradients alone)
        if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_bsums<4>), dim3(item_blocks(a)), dim3(NM_THREADS), 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_bsums<1>), dim3(item_blocks(a)), dim3(NM_THREADS), 0, st, a);
        if (a.sums == 3) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_bfinish<3>), finish_blocks(a), dim3(NM_THREADS), 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_bfinish<2>), finish_blocks(a), dim3(NM_THREADS), 0, st, a);
        launches += 2;
    }
    if (g.out || params) {   // (without gx the pass ends behind the parameter gradients)
        if (a.d.vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_bapply<4>), dim3(apply_blocks(a)), dim3(NM_THREADS), 0, st, a);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_nm_bapply<1>), dim3(apply_blocks(a)), dim3(NM_THREADS), 0, st, a);
        ++launches;
    }
    RLAP_HIPCHK(hipGetLastError());
    report(rep, a, launches);
    return RLAP_OK;
}

}  // namespace rlap
