// rlap_stats.hip -- snapshot statistics (rlap_snapshot_stats): for every segment of a Schur-complement result, its
// node count and the largest eigenvalue of its adjacency matrix by Lanczos in float64.  A translation unit of its own: it shares
// no device function with the elimination kernels (their register and LDS budgets are read back by tests/test_cabi_symbols.py).
//
// The column pass (rlap_snapshot.hip) checks the layout and numbers the blocks over the whole call, so segment s owns blocks
// [sb[s], sb[s+1]) and its Lanczos vectors are the entries [sb[s], sb[s+1]) of vectors of B (= blocks of all segments) doubles.  y = A x is then
// y[b] = sum over the rows r of block b of w_r * x[rb[r]], with rb[r] the block of row r's id: a segmented reduction in a fixed
// order, no atomics.  Every floating-point reduction below runs in a fixed order (lane strides, xor butterflies, four wave
// partials added in one order), so a call gives the same bits every time.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_lanczos.h"
#include "rlap_stats.h"

namespace rlap {
namespace {

constexpr int ST_THREADS = 256;       // every kernel of this file but the per-segment check
constexpr int ST_TILE = 256;          // large regime: columns per workgroup (16 groups of 16 lanes, 16 columns each)
constexpr int ST_CHECK_EVERY = 4;     // Ritz value of T_j every this many steps (and on a breakdown, and at max_iter)
constexpr int ST_CHUNK = 32;          // large regime: steps enqueued between two reads of the done count
enum { ERR_DONE = COL_ERR_WORDS, ERR_MAX_ITERS = 4, ERR_NOT_CONV = 5, ERR_WORDS = 8 };   // error words behind the column pass's

// empty segments: 0 / 0 / 0 steps, converged (lambda_max = 0 is exact)
__global__ void k_st_empty(const int64_t* __restrict__ sb, int64_t S, double* __restrict__ lam, int32_t* __restrict__ iters,
                           int32_t* __restrict__ conv) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S || sb[s + 1] != sb[s]) return;
    lam[s] = 0.0; iters[s] = 0; conv[s] = 1;
}

// sum over a 256-thread workgroup in a fixed order; every thread gets the same bits
__device__ inline double wg_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();   // (red may still be read by the previous call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// largest eigenvalue of T_k by multisection on one wave: 64 Sturm counts per round shrink the bracket 65-fold (about ten rounds
// to full precision); the invariant and the result are those of lanczos::max_eig.  Wave-uniform control flow.
__device__ double wave_max_eig(const double* a, const double* b, int k) {
    if (k == 1) return a[0];
    const int lane = threadIdx.x & 63;
    const double pm = lanczos::pivmin(b, k);
    double lo, hi;
    lanczos::bracket(a, b, k, &lo, &hi);
    for (int round = 0; round < 64; ++round) {
        const double x = lo + (hi - lo) * ((double)(lane + 1) / 65.0);
        const bool above = x > lo && x < hi && lanczos::count_below(a, b, k, x, pm) == k;
        const bool below = x > lo && x < hi && !above;
        const unsigned long long ma = __ballot(above), mb = __ballot(below);
        double nhi = hi, nlo = lo;
        if (ma) nhi = __shfl(x, __ffsll((long long)ma) - 1);
        if (mb) nlo = __shfl(x, 63 - __clzll((long long)mb));
        if (nhi == hi && nlo == lo) break;
        hi = nhi; lo = nlo;
    }
    return hi;
}

// the stopping decision after step j (T_j = alpha[0..j), beta[0..j-1); bj = beta_j): 0 go on, 1 converged, 2 stop unconverged
// (scr: 2 * max_iter doubles of scratch for the twisted factorisation, used by lane 0)
__device__ inline int lanczos_decide(const double* al, const double* be, int j, double bj, double tnorm, double tol, int max_iter,
                                     double* scr, double* theta) {
    const bool breakdown = !(bj > 64.0 * DBL_EPSILON * tnorm);
    if (!(j % ST_CHECK_EVERY == 0 || breakdown || j >= max_iter)) return 0;
    const double th = wave_max_eig(al, be, j);
    double y = 0.0;
    if ((threadIdx.x & 63) == 0) y = lanczos::last_component(al, be, j, th, scr, scr + max_iter);
    y = __shfl(y, 0);
    *theta = th;
    if (lanczos::converged(bj, y, th, tol)) return 1;
    return (breakdown || j >= max_iter) ? 2 : 0;
}

// ---------------------------------------------------------------- small regime: one workgroup runs a segment's whole Lanczos
// LDS: v (current), w (previous / the new vector, written in place: A v reads only v), then alpha, beta and 2 x scratch [max_iter]
__global__ __launch_bounds__(ST_THREADS) void k_st_lanczos_small(const int32_t* __restrict__ list, const double* __restrict__ sc,
                                                                 int weighted, const int32_t* __restrict__ bstart,
                                                                 const int32_t* __restrict__ rb, const int64_t* __restrict__ sb,
                                                                 int32_t nmax, double tol, int32_t max_iter, double* __restrict__ lam,
                                                                 int32_t* __restrict__ iters, int32_t* __restrict__ conv,
                                                                 int32_t* __restrict__ err) {
    extern __shared__ double dyn[];
    __shared__ double red[4];
    __shared__ int s_decide;
    __shared__ double s_theta;
    const int64_t s = list[blockIdx.x];
    const int64_t b0 = sb[s];
    const int n = (int)(sb[s + 1] - b0);
    if (n > nmax) return;   // (the host sized the LDS for nmax; never taken)
    double* v = dyn;
    double* w = dyn + nmax;
    double* al = dyn + 2 * (int64_t)nmax;
    double* be = al + max_iter;
    const int tid = threadIdx.x, grp = tid >> 4, gl = tid & 15;
    const double v0 = 1.0 / sqrt((double)n);
    for (int i = tid; i < n; i += ST_THREADS) { v[i] = v0; w[i] = 0.0; }
    __syncthreads();
    double bprev = 0.0, tnorm = 0.0;
    int decide = 0, j = 0;
    double theta = 0.0;
    while (true) {
        ++j;
        // w = A v - beta_{j-1} w
        for (int c = grp; c < n; c += ST_THREADS / 16) {
            const int32_t r0 = bstart[b0 + c], r1 = bstart[b0 + c + 1];
            double acc = 0.0;
            for (int32_t r = r0 + gl; r < r1; r += 16) acc += (weighted ? sc[3 * (int64_t)r + 2] : 1.0) * v[rb[r] - b0];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
            if (gl == 0) w[c] = acc - bprev * w[c];
        }
        __syncthreads();
        double p = 0.0;
        for (int i = tid; i < n; i += ST_THREADS) p += w[i] * v[i];
        const double alpha = wg_sum(p, red);
        p = 0.0;
        for (int i = tid; i < n; i += ST_THREADS) { const double t = w[i] - alpha * v[i]; w[i] = t; p += t * t; }
        const double beta = sqrt(wg_sum(p, red));
        tnorm = fmax(tnorm, fabs(alpha) + bprev + beta);
        if (tid == 0) { al[j - 1] = alpha; be[j - 1] = beta; }
        __syncthreads();
        if (tid < 64) {
            double th = 0.0;
            const int d = lanczos_decide(al, be, j, beta, tnorm, tol, max_iter, be + max_iter, &th);
            if (tid == 0) { s_decide = d; s_theta = th; }
        }
        __syncthreads();
        decide = s_decide; theta = s_theta;
        if (decide) break;
        // v_{j+1} = w / beta_j goes where w was; the old v becomes the previous vector
        for (int i = tid; i < n; i += ST_THREADS) w[i] = w[i] / beta;
        double* t = v; v = w; w = t;
        bprev = beta;
        __syncthreads();
    }
    if (tid == 0) {
        lam[s] = theta; iters[s] = j; conv[s] = decide == 1 ? 1 : 0;
        atomicMax(&err[ERR_MAX_ITERS], j);
        if (decide != 1) atomicAdd(&err[ERR_NOT_CONV], 1);
    }
}

// ---------------------------------------------------------------- large regime: every step is four launches over all large segments
// tiles: tile t covers columns [c0, c0 + 256) of large segment ls[t]; large segment l is segment lseg[l], tiles [tp[l], tp[l+1])
struct LargeTables {
    const int32_t* lseg; const int32_t* tp; const int32_t* tseg; const int32_t* tc0;
    int32_t nlarge, ntiles, max_iter;
    double* al; double* be; double* scr; double* tn; int32_t* done; double* part;   // part: [2][ntiles]; scr: [nlarge][2 * max_iter]
};

// sum of part[tp[l] .. tp[l+1]) over the workgroup, in a fixed order (every tile of segment l gets the same bits)
__device__ inline double seg_sum(const double* __restrict__ part, int32_t t0, int32_t t1, double* red) {
    double p = 0.0;
    for (int32_t t = t0 + (int32_t)threadIdx.x; t < t1; t += ST_THREADS) p += part[t];
    return wg_sum(p, red);
}

// step j, part 1: w = A v - beta_{j-1} w for the tile's columns, partial w . v
__global__ __launch_bounds__(ST_THREADS) void k_st_lz_spmv(LargeTables L, int32_t j, const double* __restrict__ sc, int weighted,
                                                           const int32_t* __restrict__ bstart, const int32_t* __restrict__ rb,
                                                           const int64_t* __restrict__ sb, const double* __restrict__ v,
                                                           double* __restrict__ w) {
    __shared__ double red[4];
    const int32_t t = blockIdx.x;
    const int32_t l = L.tseg[t];
    if (L.done[l]) return;
    const int64_t s = L.lseg[l];
    const int64_t b0 = sb[s], n = sb[s + 1] - b0;
    const double bprev = j > 1 ? L.be[(int64_t)l * L.max_iter + j - 2] : 0.0;
    const int tid = threadIdx.x, grp = tid >> 4, gl = tid & 15;
    const int64_t c0 = L.tc0[t], c1 = std::min<int64_t>(c0 + ST_TILE, n);
    double p = 0.0;
    for (int64_t c = c0 + grp; c < c1; c += ST_THREADS / 16) {
        const int64_t b = b0 + c;
        const int32_t r0 = bstart[b], r1 = bstart[b + 1];
        double acc = 0.0;
        for (int32_t r = r0 + gl; r < r1; r += 16) acc += (weighted ? sc[3 * (int64_t)r + 2] : 1.0) * v[rb[r]];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 16);
        if (gl == 0) { const double x = acc - bprev * w[b]; w[b] = x; p += x * v[b]; }
    }
    const double tot = wg_sum(p, red);
    if (tid == 0) L.part[t] = tot;
}

// part 2: alpha_j from the partials; w -= alpha_j v; partial |w|^2
__global__ __launch_bounds__(ST_THREADS) void k_st_lz_axpy(LargeTables L, int32_t j, const int64_t* __restrict__ sb,
                                                           const double* __restrict__ v, double* __restrict__ w) {
    __shared__ double red[4];
    const int32_t t = blockIdx.x;
    const int32_t l = L.tseg[t];
    if (L.done[l]) return;
    const double alpha = seg_sum(L.part, L.tp[l], L.tp[l + 1], red);
    const int64_t s = L.lseg[l];
    const int64_t b0 = sb[s], n = sb[s + 1] - b0;
    const int64_t c0 = L.tc0[t], c1 = std::min<int64_t>(c0 + ST_TILE, n);
    double p = 0.0;
    const int64_t c = c0 + threadIdx.x;
    if (c < c1) { const double x = w[b0 + c] - alpha * v[b0 + c]; w[b0 + c] = x; p = x * x; }
    const double tot = wg_sum(p, red);
    if (threadIdx.x == 0) {
        L.part[L.ntiles + t] = tot;
        if (t == L.tp[l]) L.al[(int64_t)l * L.max_iter + j - 1] = alpha;
    }
}

// part 3: beta_j from the partials; w /= beta_j (w becomes v_{j+1}; the host swaps the roles of the two vectors)
__global__ __launch_bounds__(ST_THREADS) void k_st_lz_scale(LargeTables L, int32_t j, const int64_t* __restrict__ sb, double* __restrict__ w) {
    __shared__ double red[4];
    const int32_t t = blockIdx.x;
    const int32_t l = L.tseg[t];
    if (L.done[l]) return;
    const double beta = sqrt(seg_sum(L.part + L.ntiles, L.tp[l], L.tp[l + 1], red));
    const int64_t s = L.lseg[l];
    const int64_t b0 = sb[s], n = sb[s + 1] - b0;
    const int64_t c = L.tc0[t] + threadIdx.x;
    if (c < n && beta > 0.0) w[b0 + c] = w[b0 + c] / beta;
    if (threadIdx.x == 0 && t == L.tp[l]) L.be[(int64_t)l * L.max_iter + j - 1] = beta;
}

// part 4: one wave per large segment: the stopping decision
__global__ __launch_bounds__(64) void k_st_lz_check(LargeTables L, int32_t j, double tol, double* __restrict__ lam,
                                                    int32_t* __restrict__ iters, int32_t* __restrict__ conv, int32_t* __restrict__ err) {
    const int32_t l = blockIdx.x;
    if (L.done[l]) return;
    const double* al = L.al + (int64_t)l * L.max_iter;
    const double* be = L.be + (int64_t)l * L.max_iter;
    const double bprev = j > 1 ? be[j - 2] : 0.0;
    const double tnorm = fmax(L.tn[l], fabs(al[j - 1]) + bprev + be[j - 1]);
    double th = 0.0;
    const int d = lanczos_decide(al, be, j, be[j - 1], tnorm, tol, L.max_iter, L.scr + (int64_t)l * 2 * L.max_iter, &th);
    if (threadIdx.x != 0) return;
    L.tn[l] = tnorm;
    if (!d) return;
    const int64_t s = L.lseg[l];
    lam[s] = th; iters[s] = j; conv[s] = d == 1 ? 1 : 0;
    L.done[l] = 1;
    atomicAdd(&err[ERR_DONE], 1);
    atomicMax(&err[ERR_MAX_ITERS], j);
    if (d != 1) atomicAdd(&err[ERR_NOT_CONV], 1);
}

struct Bufs {
    ColumnBufs col;
    int32_t* stage;
    double *v0, *v1, *part, *al, *be, *scr, *tn;
    int32_t* done;
};

struct Dims {
    int64_t idx_n, bcap, lcap, tcap, stage_n;
};

Dims dims_of(int64_t m, int64_t S, int64_t G, int64_t N) {
    Dims d;
    d.idx_n = (S / G) * N;
    d.bcap = std::min<int64_t>(m, d.idx_n);
    d.lcap = std::min<int64_t>(S, d.bcap / (STATS_SMALL_MAX + 1));
    d.tcap = d.bcap / ST_TILE + d.lcap;
    d.stage_n = S + 2 * d.lcap + 1 + 2 * d.tcap;   // small list, lseg, tp, tseg, tc0
    return d;
}

size_t carve_stats(Carve& C, int64_t m, int64_t S, int64_t G, int64_t N, int32_t max_iter, Bufs& B) {
    const Dims d = dims_of(m, S, G, N);
    C.off = column_pass_carve(C.base, C.off, m, S, G, N, ERR_WORDS, &B.col);
    B.stage = C.take<int32_t>(d.stage_n);
    const int64_t vb = d.lcap > 0 ? d.bcap : 0;   // (vectors of the large regime only)
    B.v0 = C.take<double>(vb);
    B.v1 = C.take<double>(vb);
    B.part = C.take<double>(2 * d.tcap);
    B.al = C.take<double>(d.lcap * max_iter);
    B.be = C.take<double>(d.lcap * max_iter);
    B.scr = C.take<double>(d.lcap * 2 * max_iter);
    B.tn = C.take<double>(d.lcap);
    B.done = C.take<int32_t>(d.lcap);
    return C.off + 256;
}

__global__ void k_st_fill_large(const int32_t* __restrict__ lseg, int32_t nlarge, const int64_t* __restrict__ sb,
                                double* __restrict__ v, double* __restrict__ w, double* __restrict__ tn, int32_t* __restrict__ done) {
    const int32_t l = blockIdx.y;
    const int64_t s = lseg[l];
    const int64_t b0 = sb[s], n = sb[s + 1] - b0;
    const double v0 = 1.0 / sqrt((double)n);
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
        v[b0 + c] = v0; w[b0 + c] = 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { tn[l] = 0.0; done[l] = 0; }
}

}  // namespace

size_t snapshot_stats_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int32_t max_iter) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_stats(C, m, S, G, N, max_iter, B);
}

int snapshot_stats_run(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotStatsArgs& a, SnapshotStatsReport* rep) {
    *rep = SnapshotStatsReport{};
    const SnapshotSeg& in = a.seg;
    const int64_t m = in.m, S = in.S, G = in.G, N = in.N;
    // 1. the tables, read back and checked
    std::vector<int64_t> hptr, hnp;
    int rc = read_tables_checked(st, in.ptr, S, m, in.node_ptr, G, N, &hptr, &hnp);
    rep->host_syncs = 1;
    if (rc != RLAP_OK) return rc;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_stats(C, m, S, G, N, a.max_iter, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const Dims d = dims_of(m, S, G, N);
    if (m == 0) {
        RLAP_HIPCHK(hipMemsetAsync(a.nodes, 0, sizeof(int64_t) * (size_t)S, st));
        RLAP_HIPCHK(hipMemsetAsync(a.lambda_max, 0, sizeof(double) * (size_t)S, st));
        RLAP_HIPCHK(hipMemsetAsync(a.iters, 0, sizeof(int32_t) * (size_t)S, st));
        std::vector<int32_t> ones((size_t)S, 1);
        RLAP_HIPCHK(hipMemcpyAsync(a.converged, ones.data(), sizeof(int32_t) * (size_t)S, hipMemcpyHostToDevice, st));
        RLAP_HIPCHK(hipStreamSynchronize(st));
        rep->host_syncs += 1;
        return RLAP_OK;
    }
    // 2. the column pass
    RLAP_HIPCHK(hipMemsetAsync(B.col.err, 0, sizeof(int32_t) * ERR_WORDS, st));
    rc = column_pass_enqueue(st, in.sc, m, in.ptr, S, in.node_ptr, G, N, B.col, a.nodes);
    if (rc != RLAP_OK) return rc;
    // 3. node counts and the layout checks, read back once
    std::vector<int64_t> hnodes((size_t)S);
    int32_t herr[ERR_WORDS];
    RLAP_HIPCHK(hipMemcpyAsync(hnodes.data(), a.nodes, sizeof(int64_t) * (size_t)S, hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipMemcpyAsync(herr, B.col.err, sizeof(herr), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs += 1;
    rc = layout_status(herr);
    if (rc != RLAP_OK) return rc;
    // 4. the regimes
    std::vector<int32_t> stage((size_t)d.stage_n, 0);
    int32_t nsmall = 0, nlarge = 0, ntiles = 0, nmax = 1;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t n = hnodes[(size_t)s];
        if (n > 0 && n <= STATS_SMALL_MAX) { stage[(size_t)nsmall++] = (int32_t)s; nmax = std::max<int32_t>(nmax, (int32_t)n); }
    }
    int32_t* lseg = stage.data() + S;
    int32_t* tp = lseg + d.lcap;
    int32_t* tseg = tp + d.lcap + 1;
    int32_t* tc0 = tseg + d.tcap;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t n = hnodes[(size_t)s];
        if (n <= STATS_SMALL_MAX) continue;
        if (nlarge >= d.lcap) return RLAP_E_INTERNAL;
        tp[nlarge] = ntiles;
        lseg[nlarge] = (int32_t)s;
        for (int64_t c = 0; c < n; c += ST_TILE) {
            if (ntiles >= d.tcap) return RLAP_E_INTERNAL;
            tseg[ntiles] = nlarge; tc0[ntiles] = (int32_t)c; ++ntiles;
        }
        ++nlarge;
    }
    tp[nlarge] = ntiles;
    rep->small_segments = nsmall; rep->large_segments = nlarge;
    RLAP_HIPCHK(hipMemcpyAsync(B.stage, stage.data(), sizeof(int32_t) * (size_t)d.stage_n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_st_empty, dim3(grid_blocks(S, 256)), dim3(256), 0, st, B.col.sb, S, a.lambda_max, a.iters, a.converged);
    RLAP_HIPCHK(hipGetLastError());
    if (nsmall > 0) {
        const size_t lds = sizeof(double) * (2 * (size_t)nmax + 4 * (size_t)a.max_iter);
        RLAP_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_st_lanczos_small), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_st_lanczos_small, dim3((unsigned)nsmall), dim3(ST_THREADS), lds, st, B.stage, in.sc, a.weighted, B.col.bstart, B.col.rb,
                           B.col.sb, nmax, a.tol, a.max_iter, a.lambda_max, a.iters, a.converged, B.col.err);
        RLAP_HIPCHK(hipGetLastError());
    }
    int64_t steps = 0;
    if (nlarge > 0) {
        LargeTables L;
        L.lseg = B.stage + S; L.tp = L.lseg + d.lcap; L.tseg = L.tp + d.lcap + 1; L.tc0 = L.tseg + d.tcap;
        L.nlarge = nlarge; L.ntiles = ntiles; L.max_iter = a.max_iter;
        L.al = B.al; L.be = B.be; L.scr = B.scr; L.tn = B.tn; L.done = B.done; L.part = B.part;
        hipLaunchKernelGGL(k_st_fill_large, dim3(64, (unsigned)nlarge), dim3(256), 0, st, L.lseg, nlarge, B.col.sb, B.v0, B.v1, B.tn, B.done);
        RLAP_HIPCHK(hipGetLastError());
        for (int32_t j0 = 1; j0 <= a.max_iter; j0 += ST_CHUNK) {
            const int32_t j1 = std::min<int32_t>(j0 + ST_CHUNK - 1, a.max_iter);
            for (int32_t j = j0; j <= j1; ++j) {
                double* v = (j & 1) ? B.v0 : B.v1;   // v_j; the other vector holds v_{j-1} and receives v_{j+1}
                double* w = (j & 1) ? B.v1 : B.v0;
                hipLaunchKernelGGL(k_st_lz_spmv, dim3((unsigned)ntiles), dim3(ST_THREADS), 0, st, L, j, in.sc, a.weighted, B.col.bstart, B.col.rb, B.col.sb, v, w);
                hipLaunchKernelGGL(k_st_lz_axpy, dim3((unsigned)ntiles), dim3(ST_THREADS), 0, st, L, j, B.col.sb, v, w);
                hipLaunchKernelGGL(k_st_lz_scale, dim3((unsigned)ntiles), dim3(ST_THREADS), 0, st, L, j, B.col.sb, w);
                hipLaunchKernelGGL(k_st_lz_check, dim3((unsigned)nlarge), dim3(64), 0, st, L, j, a.tol, a.lambda_max, a.iters, a.converged, B.col.err);
                rep->large_launches += 4;
            }
            RLAP_HIPCHK(hipGetLastError());
            int32_t ndone = 0;
            RLAP_HIPCHK(hipMemcpyAsync(&ndone, B.col.err + ERR_DONE, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            RLAP_HIPCHK(hipStreamSynchronize(st));
            rep->host_syncs += 1;
            steps = j1;
            if (ndone >= nlarge) break;
        }
    }
    // 5. what the call reports
    RLAP_HIPCHK(hipMemcpyAsync(herr, B.col.err, sizeof(herr), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs += 1;
    rep->lanczos_steps = herr[ERR_MAX_ITERS];
    rep->large_steps = steps;
    rep->not_converged = herr[ERR_NOT_CONV];
    return RLAP_OK;
}

}  // namespace rlap
