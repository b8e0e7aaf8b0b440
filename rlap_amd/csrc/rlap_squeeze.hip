// rlap_squeeze.hip -- the squeeze pass (rlap_squeeze.h).  Four grid-wide kernels, none persistent, plain loads and
// stores: rank (live entries of every surviving column numbered in traversal order), a prefix sum of the counts (the new column
// pointers), copy (rlap_core.h::squeeze_entry per live entry), epilogue (appended entries, pool, per-graph flags).
#include <algorithm>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "rlap_core.h"
#include "rlap_kernels.h"
#include "rlap_squeeze.h"

namespace rlap {

namespace {

// the input checks of the setup kernels, as the round kernel reads them
__device__ __forceinline__ bool sq_bad_input(const int32_t* __restrict__ in_flags, const double* __restrict__ in_acc) {
    return in_flags[FLAG_RANGE] || in_flags[FLAG_CROSS] || in_flags[FLAG_PERM] || in_acc[2] != 0.0 || !(in_acc[0] <= 1e-24 * in_acc[1]);
}

// A wave walks column v in traversal order, 64 slots at a time: f(slot, valid) is called by all 64 lanes together (ballots inside
// it are wave-wide); lane l of a step holds the l-th slot of that step.
template <class F>
__device__ __forceinline__ void wave_col_slots(const Arrays& A, int32_t v, int lane, F f) {
    auto piece = [&](int32_t hi, int32_t lo) {   // slots hi, hi - 1, .., lo
        for (int32_t s0 = hi; s0 >= lo; s0 -= 64) { const int32_t s = s0 - lane; f(s, s >= lo); }
    };
    const int32_t a = A.vr[v].app_cnt;
    if (a > 0) {
        int32_t base = A.vr[v].app_chunk;
        int c = chunk_of(a - 1);
        int32_t idx = a - 1;
        while (idx >= 0 && base >= 0 && base < A.slot_cap) {
            const int32_t cs = chunk_start(c);
            piece(base + 1 + (idx - cs), base + 1);
            idx = cs - 1;
            base = A.e[base].nbr;
            --c;
        }
    }
    piece(A.colptr[v + 1] - 1, A.colptr[v]);
}

// Rank, short tier: one thread per vertex.  Eliminated vertices, rejected input and failed graphs count 0; long columns are listed.
__global__ __launch_bounds__(256) void k_sq_rank(Arrays A, int32_t N, const int32_t* __restrict__ vgraph, const GraphDesc* __restrict__ gd,
                                                 const int32_t* __restrict__ in_flags, const double* __restrict__ in_acc,
                                                 int32_t* __restrict__ rank, int32_t* __restrict__ cnt, int32_t* __restrict__ longlist,
                                                 int32_t* __restrict__ nlong) {
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > N) return;
    if (v == N) { cnt[N] = 0; return; }
    int32_t c = 0;
    if (A.vr[v].pqpos != -2 && !sq_bad_input(in_flags, in_acc) && gd[vgraph[v]].status == 0) {
        const int32_t ext = (A.colptr[v + 1] - A.colptr[v]) + A.vr[v].app_cnt;
        if (ext > SQ_SHORT) { longlist[atomicAdd(nlong, 1)] = v; return; }   // (its count: k_sq_rank_long)
        c = squeeze_rank_col(A, v, rank);
    }
    cnt[v] = c;
}

// Rank, long tier: one wave per listed column, ballot prefix sums over 64 slots at a time.
__global__ __launch_bounds__(256) void k_sq_rank_long(Arrays A, const int32_t* __restrict__ longlist, const int32_t* __restrict__ nlong,
                                                      int32_t* __restrict__ rank, int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int32_t nw = (int32_t)(gridDim.x * (blockDim.x >> 6));
    const int32_t n = *nlong;
    for (int32_t i = (int32_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); i < n; i += nw) {
        const int32_t v = longlist[i];
        int32_t run = 0;
        wave_col_slots(A, v, lane, [&](int32_t s, bool valid) {
            const bool live = valid && A.e[s].val > 0;
            const unsigned long long m = __ballot(live);
            if (live) rank[s] = run + __popcll(m & ((1ull << lane) - 1ull));
            run += __popcll(m);
        });
        if (lane == 0) cnt[v] = run;
    }
}

// Copy, short tier.  A column without live entries (eliminated, rejected, failed, or simply empty) has nothing to copy.
__global__ __launch_bounds__(256) void k_sq_copy(Arrays A, int32_t N, const int32_t* __restrict__ vgraph, GraphDesc* __restrict__ gd,
                                                 const int32_t* __restrict__ rank, const int32_t* __restrict__ colptr2, Slot* __restrict__ e2) {
    const int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    if (colptr2[v + 1] == colptr2[v]) return;
    if ((A.colptr[v + 1] - A.colptr[v]) + A.vr[v].app_cnt > SQ_SHORT) return;   // (k_sq_copy_long)
    bool ok = true;
    col_for_each_slot(A, v, [&](int32_t s) { if (A.e[s].val > 0) ok &= squeeze_entry(A, rank, colptr2, e2, N, v, s); });
    if (!ok) atomicMax(&gd[vgraph[v]].status, (int32_t)ST_INTERNAL);
}

__global__ __launch_bounds__(256) void k_sq_copy_long(Arrays A, int32_t N, const int32_t* __restrict__ vgraph, GraphDesc* __restrict__ gd,
                                                      const int32_t* __restrict__ longlist, const int32_t* __restrict__ nlong,
                                                      const int32_t* __restrict__ rank, const int32_t* __restrict__ colptr2, Slot* __restrict__ e2) {
    const int lane = threadIdx.x & 63;
    const int32_t nw = (int32_t)(gridDim.x * (blockDim.x >> 6));
    const int32_t n = *nlong;
    for (int32_t i = (int32_t)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); i < n; i += nw) {
        const int32_t v = longlist[i];
        bool ok = true;
        wave_col_slots(A, v, lane, [&](int32_t s, bool valid) { if (valid && A.e[s].val > 0) ok &= squeeze_entry(A, rank, colptr2, e2, N, v, s); });
        if (!ok) atomicMax(&gd[vgraph[v]].status, (int32_t)ST_INTERNAL);
    }
}

// Epilogue: no column has appended entries any more, the pool restarts behind the new segments (the live entries never exceed the
// input's), and every graph gives up its pool reservation and its hand-over flag -- the next launch of the 16-slot kernel tries again.
__global__ __launch_bounds__(256) void k_sq_epilogue(VRec* __restrict__ vr, int32_t N, const int32_t* __restrict__ colptr2, int32_t* __restrict__ pool_top,
                                                     GraphDesc* __restrict__ gd, int32_t G, int32_t* __restrict__ marks) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) { vr[i].app_cnt = 0; vr[i].app_chunk = -1; }
    if (i < G) { gd[i].pool_cur = 0; gd[i].pool_end = 0; gd[i].narrow = 0; marks[i] = gd[i].narrow_rounds; }
    if (i == 0) *pool_top = colptr2[N];
}

}  // namespace

int squeeze_scan_tmp_bytes(int64_t N, size_t* bytes) {
    size_t b = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, b, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)(N + 1), rocprim::plus<int32_t>(), (hipStream_t) nullptr);
    *bytes = b;
    return (int)e;
}

int launch_squeeze(hipStream_t stream, const Arrays& A, const SqueezeBufs& Q, int pass, Slot* e_dst, int32_t* colptr_dst, GraphDesc* gd, int32_t G,
                   const int32_t* in_flags, const double* in_acc) {
    const int32_t N = Q.N;
    const unsigned nb = (unsigned)((N + 1 + 255) / 256);
    const unsigned nb_long = 1024;   // 4096 waves over the listed columns
    hipError_t e = hipMemsetAsync(Q.nlong, 0, sizeof(int32_t), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_sq_rank, dim3(nb), dim3(256), 0, stream, A, N, Q.vgraph, gd, in_flags, in_acc, Q.rank, Q.cnt, Q.longlist, Q.nlong);
    hipLaunchKernelGGL(k_sq_rank_long, dim3(nb_long), dim3(256), 0, stream, A, Q.longlist, Q.nlong, Q.rank, Q.cnt);
    size_t bytes = Q.scan_tmp_bytes;
    e = rocprim::exclusive_scan(Q.scan_tmp, bytes, Q.cnt, colptr_dst, (int32_t)0, (size_t)(N + 1), rocprim::plus<int32_t>(), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_sq_copy, dim3(nb), dim3(256), 0, stream, A, N, Q.vgraph, gd, Q.rank, colptr_dst, e_dst);
    hipLaunchKernelGGL(k_sq_copy_long, dim3(nb_long), dim3(256), 0, stream, A, N, Q.vgraph, gd, Q.longlist, Q.nlong, Q.rank, colptr_dst, e_dst);
    const unsigned nbe = (unsigned)((std::max<int32_t>(N, G) + 255) / 256);
    hipLaunchKernelGGL(k_sq_epilogue, dim3(nbe), dim3(256), 0, stream, A.vr, N, colptr_dst, A.pool_top, gd, G, Q.marks + (size_t)pass * (size_t)G);
    return (int)hipGetLastError();
}

}  // namespace rlap
