// rlap_featlin.hip -- the sparse first layer (rlap_feature_count / rlap_feature_plan_build / rlap_feature_plan_apply):
// a dense (N, Fin) feature matrix as the lists of rlap_featlin.h, built once, and the products (x * keep[k]) @ W for K views and
// dW = sum_k keep[k] * (x^T G[k]) over them.  A translation unit of its own: no device function is shared with rlap_plan.hip, whose
// planned call is the model of the kernels below.
//
// The build
//   forward     one wave per (row, block of FL_COLS columns): the kept entries counted; rocPRIM's exclusive scan of the counts in
//               (row, block) order; off[i] is the scan at the row's first block; the fill walks a block 64 columns at a time and
//               ranks the kept ones by a ballot, so the records of a row come by ascending column.
//   transposed  one lane per (block of FL_ROWS rows, column): the kept entries counted; the scan in (column, block) order; off[j]
//               is the scan at the column's first block; the fill walks the block's rows in order, so the records of a column come
//               by ascending row.
//   lists       per slot: the chunks of a long list; their scan; the directory.  The longest list and the long lists are counted
//               (integer atomics on counters only).
//   One read-back: both recounts, the chunk totals, the counters.
// The planned call
//   masks       one 32-bit word per column: bit k = keep[k][j] != 0 (all ones without d_keep).
//   forward     one group of up to 64 lanes per (row, feature tile).  One walk over the row's records serves up to VIEW_GROUP views:
//               per turn four records, their keep words and their rows of W (each loaded once), then the adds of every view by a
//               select on its bit.  More views run in groups of VIEW_GROUP.  A row longer than CHUNK is summed chunk by chunk by
//               the same group.
//   transposed  chunk sums per (directory entry, kept view, feature tile) to part[] (arena), then one group per (column, feature
//               tile): for the views that keep the column, in view order, the chunk sums in chunk order (or, past the part[]
//               budget, summed on the spot).
// Everything a planned call reads from the plan is clamped before it is used as an index.  No LDS, no atomic on a float.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_featlin.h"
#include "rlap_featlin_api.h"
#include "rlap_plan.h"
#include "rlap_spmm.h"

namespace rlap {
namespace {

constexpr int FL_THREADS = 256;
constexpr int64_t FL_MAX_GRID = (int64_t)1 << 20;        // workgroups of a launch (the kernels stride over their tasks)
constexpr int64_t FL_PART_BYTES = (int64_t)256 << 20;    // budget of the chunk sums (rlap_spmm.hip's)
constexpr int64_t FL_PART_MIN = 4096;                    // directory entries whose chunk sums always fit
constexpr int FL_TURN = 4;                               // records of a turn
constexpr int64_t FL_COLS = 1024;                        // columns of a forward count block (one wave)
constexpr int64_t FL_ROWS = 64;                          // rows of a transposed count block (one lane per column)
enum { CNT_LONG_F = 0, CNT_LONG_T = 1, CNT_MAX_F = 2, CNT_MAX_T = 3, CNT_WORDS = 4 };

inline unsigned fl_blocks(int64_t n, int bs) { return capped_blocks(n, bs, FL_MAX_GRID); }
inline int64_t fl_col_blocks(int64_t Fin) { return (Fin + FL_COLS - 1) / FL_COLS; }
inline int64_t fl_row_blocks(int64_t N) { return (N + FL_ROWS - 1) / FL_ROWS; }

// ------------------------------------------------------------------------------------------------ the build
// cnt[i * nb + b] = kept entries of row i in columns [b * FL_COLS, (b + 1) * FL_COLS); one entry behind the last is 0
template <class X>
__global__ __launch_bounds__(FL_THREADS) void k_fl_count_rows(const X* __restrict__ x, int64_t N, int64_t Fin, int64_t nb, int32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t tasks = N * nb, nwaves = ((int64_t)gridDim.x * FL_THREADS) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[tasks] = 0;
    for (int64_t t = ((int64_t)blockIdx.x * FL_THREADS + threadIdx.x) >> 6; t < tasks; t += nwaves) {
        const int64_t i = t / nb, b = t - i * nb;
        const int64_t j0 = b * FL_COLS, j1 = std::min<int64_t>(j0 + FL_COLS, Fin);
        int c = 0;
        for (int64_t j = j0 + lane; j < j1; j += 64) c += featlin::kept((double)x[i * Fin + j]) ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
        if (lane == 0) cnt[t] = c;
    }
}

// the forward records: a block's kept entries from pos[t] on, ranked by a ballot; nothing is written outside rec[0, cap)
template <class X>
__global__ __launch_bounds__(FL_THREADS) void k_fl_fill_rows(const X* __restrict__ x, int64_t N, int64_t Fin, int64_t nb,
                                                             const int64_t* __restrict__ pos, plan::Record* __restrict__ rec, int64_t cap) {
    const int lane = threadIdx.x & 63;
    const int64_t tasks = N * nb, nwaves = ((int64_t)gridDim.x * FL_THREADS) >> 6;
    for (int64_t t = ((int64_t)blockIdx.x * FL_THREADS + threadIdx.x) >> 6; t < tasks; t += nwaves) {
        const int64_t i = t / nb, b = t - i * nb;
        const int64_t j0 = b * FL_COLS, j1 = std::min<int64_t>(j0 + FL_COLS, Fin);
        int64_t base = pos[t];
        for (int64_t jt = j0; jt < j1; jt += 64) {   // (jt is the wave's: every lane takes part in the ballot)
            const int64_t j = jt + lane;
            const double v = j < j1 ? (double)x[i * Fin + j] : 0.0;
            const bool k = j < j1 && featlin::kept(v);
            const unsigned long long vote = __ballot(k);
            const int64_t at = base + __popcll(vote & (((unsigned long long)1 << lane) - 1));
            if (k && at >= 0 && at < cap) rec[at] = plan::Record{v, (int32_t)j, 0};
            base += __popcll(vote);
        }
    }
}

// cnt[j * nrb + rb] = kept entries of column j in rows [rb * FL_ROWS, (rb + 1) * FL_ROWS); one entry behind the last is 0
template <class X>
__global__ __launch_bounds__(FL_THREADS) void k_fl_count_cols(const X* __restrict__ x, int64_t N, int64_t Fin, int64_t nrb, int32_t* __restrict__ cnt) {
    const int64_t tasks = nrb * Fin;
    if (blockIdx.x == 0 && threadIdx.x == 0) cnt[tasks] = 0;
    for (int64_t t = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; t < tasks; t += (int64_t)gridDim.x * FL_THREADS) {
        const int64_t rb = t / Fin, j = t - rb * Fin;
        const int64_t i0 = rb * FL_ROWS, i1 = std::min<int64_t>(i0 + FL_ROWS, N);
        int c = 0;
        for (int64_t i = i0; i < i1; ++i) c += featlin::kept((double)x[i * Fin + j]) ? 1 : 0;
        cnt[j * nrb + rb] = c;
    }
}

// the transposed records: a (column, block of rows)'s kept entries from pos[j * nrb + rb] on, in row order
template <class X>
__global__ __launch_bounds__(FL_THREADS) void k_fl_fill_cols(const X* __restrict__ x, int64_t N, int64_t Fin, int64_t nrb,
                                                             const int64_t* __restrict__ pos, plan::Record* __restrict__ rec, int64_t cap) {
    const int64_t tasks = nrb * Fin;
    for (int64_t t = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; t < tasks; t += (int64_t)gridDim.x * FL_THREADS) {
        const int64_t rb = t / Fin, j = t - rb * Fin;
        const int64_t i0 = rb * FL_ROWS, i1 = std::min<int64_t>(i0 + FL_ROWS, N);
        int64_t at = pos[j * nrb + rb];
        for (int64_t i = i0; i < i1; ++i) {
            const double v = (double)x[i * Fin + j];
            if (!featlin::kept(v)) continue;
            if (at >= 0 && at < cap) rec[at] = plan::Record{v, (int32_t)i, 0};
            ++at;
        }
    }
}

// off[s] = pos[s * stride], s in [0, slots]: the scan at a slot's first block, and the total behind the last
__global__ void k_fl_offsets(const int64_t* __restrict__ pos, int64_t stride, int64_t slots, int64_t* __restrict__ off) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= slots; s += (int64_t)gridDim.x * blockDim.x) off[s] = pos[s * stride];
}

// per slot (and one entry behind the last): the chunks of a long list; the long lists and the longest list counted
__global__ void k_fl_lists(const int64_t* __restrict__ off, int64_t slots, int32_t* __restrict__ nch, unsigned long long* __restrict__ cnt, int d) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= slots; s += (int64_t)gridDim.x * blockDim.x) {
        const int64_t len = s < slots ? std::max<int64_t>(off[s + 1] - off[s], 0) : 0;
        const int64_t nc = plan::dir_chunks(len);
        nch[s] = (int32_t)nc;
        if (nc > 0) atomicAdd(&cnt[d ? CNT_LONG_T : CNT_LONG_F], 1ull);
        unsigned long long* mx = &cnt[d ? CNT_MAX_T : CNT_MAX_F];
        if ((unsigned long long)len > *mx) atomicMax(mx, (unsigned long long)len);   // (the plain read only spares atomics)
    }
}

// the directory: the (slot, chunk) of every chunk number
__global__ void k_fl_dir(const int64_t* __restrict__ off, int64_t slots, const int32_t* __restrict__ nch, const int64_t* __restrict__ choff,
                         plan::ChunkRef* __restrict__ dir, int64_t dcap) {
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += (int64_t)gridDim.x * blockDim.x) {
        if (nch[s] == 0) continue;
        plan::dir_write(s, off[s + 1] - off[s], choff[s], dcap, [&](int64_t q, plan::ChunkRef c) { dir[q] = c; });
    }
}

struct Bufs {
    unsigned long long* cnt;
    int32_t* bcnt[2]; int64_t* bpos[2]; int64_t blocks[2];   // per direction: counts and their scan, [blocks + 1]
    int32_t* nch; int64_t* choff[2];
    void* scan_tmp; size_t scan_bytes;
};

size_t carve_build(Carve& C, int64_t N, int64_t Fin, int flags, Bufs& B) {
    const bool want[2] = {(flags & RLAP_PLAN_FORWARD) != 0, (flags & RLAP_PLAN_TRANSPOSED) != 0};
    const int64_t slots[2] = {N, Fin};
    B.blocks[0] = N * fl_col_blocks(Fin);
    B.blocks[1] = Fin * fl_row_blocks(N);
    B.cnt = C.take<unsigned long long>(CNT_WORDS);
    int64_t longest = std::max(N, Fin) + 1;
    for (int d = 0; d < 2; ++d) {
        B.bcnt[d] = C.take<int32_t>(want[d] ? B.blocks[d] + 1 : 0);
        B.bpos[d] = C.take<int64_t>(want[d] ? B.blocks[d] + 1 : 0);
        B.choff[d] = C.take<int64_t>(want[d] ? slots[d] + 1 : 0);
        if (want[d]) longest = std::max(longest, B.blocks[d] + 1);
    }
    B.nch = C.take<int32_t>(std::max(N, Fin) + 1);
    B.scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, B.scan_bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)longest,
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    B.scan_tmp = C.take<char>((int64_t)B.scan_bytes);
    return C.off + 256;
}

template <class X>
int build_lists(hipStream_t st, const X* x, int64_t N, int64_t Fin, int d, const Bufs& B, int64_t* off, plan::Record* rec, int64_t cap) {
    const int64_t blocks = B.blocks[d];
    size_t sb = B.scan_bytes;
    if (d == plan::FORWARD) {
        const int64_t nb = fl_col_blocks(Fin);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_count_rows<X>), dim3(fl_blocks(blocks * 64, FL_THREADS)), dim3(FL_THREADS), 0, st, x, N, Fin, nb, B.bcnt[d]);
        RLAP_HIPCHK(hipGetLastError());
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, sb, B.bcnt[d], B.bpos[d], (int64_t)0, (size_t)(blocks + 1), rocprim::plus<int64_t>(), st));
        hipLaunchKernelGGL(k_fl_offsets, dim3(fl_blocks(N + 1, 256)), dim3(256), 0, st, B.bpos[d], nb, N, off);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_fill_rows<X>), dim3(fl_blocks(blocks * 64, FL_THREADS)), dim3(FL_THREADS), 0, st, x, N, Fin, nb, B.bpos[d], rec, cap);
    } else {
        const int64_t nrb = fl_row_blocks(N);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_count_cols<X>), dim3(fl_blocks(blocks, FL_THREADS)), dim3(FL_THREADS), 0, st, x, N, Fin, nrb, B.bcnt[d]);
        RLAP_HIPCHK(hipGetLastError());
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, sb, B.bcnt[d], B.bpos[d], (int64_t)0, (size_t)(blocks + 1), rocprim::plus<int64_t>(), st));
        hipLaunchKernelGGL(k_fl_offsets, dim3(fl_blocks(Fin + 1, 256)), dim3(256), 0, st, B.bpos[d], nrb, Fin, off);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_fill_cols<X>), dim3(fl_blocks(blocks, FL_THREADS)), dim3(FL_THREADS), 0, st, x, N, Fin, nrb, B.bpos[d], rec, cap);
    }
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// ------------------------------------------------------------------------------------------------ the planned call
struct Fu {
    const int64_t* off; const plan::Record* rec; const plan::ChunkRef* dir;
    int64_t entries, chunks;                  // records and directory entries of the direction
    int64_t slots, ids;                       // lists of the direction; a record's id lies in [0, ids)
    int64_t N, Fin, F;
    int K;
    const uint32_t* mask;                     // [Fin] bit k: view k keeps the column
    double* part; int64_t pcap;               // [pcap, K, F] chunk sums (transposed)
    int lg; int64_t ftiles;                   // log2 of the lanes of a group; groups a row of F features takes
};

// mask[j]: bit k = keep[k][j] != 0; without keep the one view keeps everything
__global__ void k_fl_mask(const uint8_t* __restrict__ keep, int K, int64_t Fin, uint32_t* __restrict__ mask) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < Fin; j += (int64_t)gridDim.x * blockDim.x) {
        uint32_t m = keep ? 0u : 1u;
        if (keep)
            for (int k = 0; k < K; ++k) m |= keep[(int64_t)k * Fin + j] ? (1u << k) : 0u;
        mask[j] = m;
    }
}

template <class T, int VEC> __device__ inline void fl_load(const T* __restrict__ p, T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = p[0];
    } else if constexpr (sizeof(T) == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const double2 q = *reinterpret_cast<const double2*>(p);
        v[0] = q.x; v[1] = q.y;
    }
}

template <class T, int VEC> __device__ inline void fl_store(T* __restrict__ p, const double (&acc)[VEC]) {
    if constexpr (VEC == 1) {
        p[0] = (T)acc[0];
    } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    } else {
        *reinterpret_cast<double2*>(p) = make_double2(acc[0], acc[1]);
    }
}

// records [k0, k1) of the list at o0, summed from 0 in list order, for KG views side by side.  FL_TURN records at a time: their
// loads back to back, then their keep words and their rows of xl back to back, then the adds; a turn past the end repeats the last
// entry's loads and keeps the sums as they were, by a select; so does a view whose bit (g0 + v of the column's word) is clear.
// Without MASKED (the transposed lists: KG is 1) every entry counts.  The add order is rlap_featlin.h's.
template <class T, int VEC, int KG, bool MASKED>
__device__ inline void fl_sum_range(const Fu& a, const T* __restrict__ xl, int g0, int64_t o0, int64_t k0, int64_t k1, int64_t f0,
                                    double (&acc)[KG][VEC]) {
#pragma unroll
    for (int g = 0; g < KG; ++g)
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[g][v] = 0.0;
    const uint4* __restrict__ recs = reinterpret_cast<const uint4*>(a.rec);
    const int32_t nmax = (int32_t)(a.ids - 1);
    for (int64_t k = k0; k < k1; k += FL_TURN) {
        uint4 q[FL_TURN];
#pragma unroll
        for (int u = 0; u < FL_TURN; ++u) q[u] = recs[o0 + (k + u < k1 ? k + u : k1 - 1)];
        __builtin_amdgcn_sched_barrier(0);
        T xv[FL_TURN][VEC];
        uint32_t bits[FL_TURN];
#pragma unroll
        for (int u = 0; u < FL_TURN; ++u) {
            const int64_t id = (int64_t)std::min(std::max((int32_t)q[u].z, 0), nmax);
            bits[u] = MASKED ? (a.mask[id] >> g0) : 1u;
            fl_load<T, VEC>(xl + id * a.F + f0, xv[u]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < FL_TURN; ++u) {
            const bool live = k + u < k1;
            const double cu = __hiloint2double((int)q[u].y, (int)q[u].x);
#pragma unroll
            for (int g = 0; g < KG; ++g) {
                const bool on = live && ((bits[u] >> g) & 1u) != 0;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double t = spmm::accumulate(acc[g][v], cu, (double)xv[u][v]);
                    acc[g][v] = on ? t : acc[g][v];
                }
            }
        }
    }
}

// the list of a slot: n records from o0 on, both clamped to the records the direction has
__device__ inline void fl_list(const Fu& a, int64_t slot, int64_t& o0, int64_t& n) {
    o0 = featlin::clamp(a.off[slot], 0, a.entries);
    n = featlin::clamp(a.off[slot + 1], o0, a.entries) - o0;
}

// y[k][i][f] for every view: KG views a pass
template <class T, int VEC, int KG>
__global__ __launch_bounds__(FL_THREADS) void k_fl_forward(Fu a, const T* __restrict__ w, T* __restrict__ y) {
    const int64_t tasks = a.slots * a.ftiles;
    const int64_t lmask = ((int64_t)1 << a.lg) - 1;
    for (int64_t gt = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; (gt >> a.lg) < tasks; gt += (int64_t)gridDim.x * FL_THREADS) {
        const int64_t task = gt >> a.lg;
        const int64_t slot = task / a.ftiles, ft = task - slot * a.ftiles;
        const int64_t f0 = (((ft << a.lg) | (gt & lmask))) * VEC;
        if (f0 >= a.F) continue;
        int64_t o0, n;
        fl_list(a, slot, o0, n);
        const int64_t nc = spmm::num_chunks(n);
        for (int g0 = 0; g0 < a.K; g0 += KG) {
            double total[KG][VEC];
#pragma unroll
            for (int g = 0; g < KG; ++g)
#pragma unroll
                for (int v = 0; v < VEC; ++v) total[g][v] = 0.0;
            for (int64_t k = 0; k < nc; ++k) {
                double acc[KG][VEC];
                fl_sum_range<T, VEC, KG, true>(a, w, g0, o0, spmm::chunk_begin(k), spmm::chunk_end(n, k), f0, acc);
#pragma unroll
                for (int g = 0; g < KG; ++g)
#pragma unroll
                    for (int v = 0; v < VEC; ++v) total[g][v] = total[g][v] + acc[g][v];
            }
#pragma unroll
            for (int g = 0; g < KG; ++g)
                if (g0 + g < a.K) fl_store<T, VEC>(y + ((int64_t)(g0 + g) * a.N + slot) * a.F + f0, total[g]);
        }
    }
}

// the chunk sums of the long transposed lists that fit part[], per kept view
template <class T, int VEC>
__global__ __launch_bounds__(FL_THREADS) void k_fl_tchunks(Fu a, const T* __restrict__ g) {
    const int64_t tasks = std::min<int64_t>(a.chunks, a.pcap) * a.K * a.ftiles;
    const int64_t lmask = ((int64_t)1 << a.lg) - 1;
    for (int64_t gt = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; (gt >> a.lg) < tasks; gt += (int64_t)gridDim.x * FL_THREADS) {
        const int64_t task = gt >> a.lg;
        const int64_t qk = task / a.ftiles, ft = task - qk * a.ftiles;
        const int64_t q = qk / a.K, k = qk - q * a.K;
        const int64_t f0 = (((ft << a.lg) | (gt & lmask))) * VEC;
        if (f0 >= a.F) continue;
        const plan::ChunkRef c = a.dir[q];
        const int64_t slot = featlin::clamp(c.slot, 0, a.slots - 1);
        if (!((a.mask[slot] >> k) & 1u)) continue;
        int64_t o0, n;
        fl_list(a, slot, o0, n);
        if (c.k < 0 || c.k >= plan::dir_chunks(n)) continue;
        double acc[1][VEC];
        fl_sum_range<T, VEC, 1, false>(a, g + k * a.N * a.F, 0, o0, spmm::chunk_begin(c.k), spmm::chunk_end(n, c.k), f0, acc);
#pragma unroll
        for (int v = 0; v < VEC; ++v) a.part[(q * a.K + k) * a.F + f0 + v] = acc[0][v];
    }
}

// every element of dW
template <class T, int VEC>
__global__ __launch_bounds__(FL_THREADS) void k_fl_trows(Fu a, const T* __restrict__ g, T* __restrict__ dw) {
    const int64_t tasks = a.slots * a.ftiles;
    const int64_t lmask = ((int64_t)1 << a.lg) - 1;
    for (int64_t gt = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; (gt >> a.lg) < tasks; gt += (int64_t)gridDim.x * FL_THREADS) {
        const int64_t task = gt >> a.lg;
        const int64_t slot = task / a.ftiles, ft = task - slot * a.ftiles;
        const int64_t f0 = (((ft << a.lg) | (gt & lmask))) * VEC;
        if (f0 >= a.F) continue;
        int64_t o0, n;
        fl_list(a, slot, o0, n);
        const int64_t nc = spmm::num_chunks(n);
        const uint32_t bits = a.mask[slot];
        int64_t q0 = a.pcap;   // (a short list has no chunk sums: its one chunk is summed here)
        if (n > spmm::CHUNK) q0 = plan::dir_first(a.chunks, slot, [&](int64_t q) { return a.dir[q].slot; });
        const bool have = q0 + nc <= a.pcap;
        double total[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) total[v] = 0.0;
        for (int k = 0; k < a.K; ++k) {
            if (!((bits >> k) & 1u)) continue;
            double s[VEC];
#pragma unroll
            for (int v = 0; v < VEC; ++v) s[v] = 0.0;
            for (int64_t c = 0; c < nc; ++c) {
                if (have) {
                    const double* __restrict__ ps = a.part + ((q0 + c) * a.K + k) * a.F + f0;
#pragma unroll
                    for (int v = 0; v < VEC; ++v) s[v] = s[v] + ps[v];
                } else {
                    double acc[1][VEC];
                    fl_sum_range<T, VEC, 1, false>(a, g + (int64_t)k * a.N * a.F, 0, o0, spmm::chunk_begin(c), spmm::chunk_end(n, c), f0, acc);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) s[v] = s[v] + acc[0][v];
                }
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) total[v] = total[v] + s[v];
        }
        fl_store<T, VEC>(dw + slot * a.F + f0, total);
    }
}

// directory entries whose chunk sums the call keeps: every one when they fit the budget
int64_t part_cap(int64_t chunks, int64_t row, int64_t limit) {
    if (chunks <= 0) return 0;
    if (limit >= 0) return std::min<int64_t>(chunks, limit);
    return std::min<int64_t>(chunks, std::max<int64_t>(FL_PART_MIN, FL_PART_BYTES / (8 * row)));
}

template <class T, int VEC>
void launch_forward(hipStream_t st, const Fu& a, unsigned nb, const T* w, T* y) {
    if (a.K <= 1) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_forward<T, VEC, 1>), dim3(nb), dim3(FL_THREADS), 0, st, a, w, y);
    else if (a.K <= 2) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_forward<T, VEC, 2>), dim3(nb), dim3(FL_THREADS), 0, st, a, w, y);
    else if (a.K <= 4) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_forward<T, VEC, 4>), dim3(nb), dim3(FL_THREADS), 0, st, a, w, y);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_forward<T, VEC, featlin::VIEW_GROUP>), dim3(nb), dim3(FL_THREADS), 0, st, a, w, y);
}

template <class T>
int launch_sums(hipStream_t st, Fu a, const FeatureApplyArgs& g, bool transpose) {
    constexpr int V = 16 / (int)sizeof(T);
    const T* w = static_cast<const T*>(g.w);
    T* out = static_cast<T*>(g.out);
    const bool vec = a.F % V == 0 && ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int64_t lanes = vec ? a.F / V : a.F;   // lanes a row takes
    a.lg = 0;
    while (a.lg < 6 && ((int64_t)1 << a.lg) < lanes) ++a.lg;
    a.ftiles = (lanes + ((int64_t)1 << a.lg) - 1) >> a.lg;
    hipLaunchKernelGGL(k_fl_mask, dim3(fl_blocks(a.Fin, 256)), dim3(256), 0, st, g.keep, a.K, a.Fin, const_cast<uint32_t*>(a.mask));
    const int64_t tasks = a.slots * a.ftiles;
    const unsigned nb = fl_blocks(tasks << a.lg, FL_THREADS);
    if (!transpose) {
        if (vec) launch_forward<T, V>(st, a, nb, w, out);
        else launch_forward<T, 1>(st, a, nb, w, out);
    } else {
        const int64_t ctasks = std::min<int64_t>(a.chunks, a.pcap) * a.K * a.ftiles;
        if (ctasks > 0) {   // (no long list, or no chunk sum kept: no chunk kernel)
            const unsigned cb = fl_blocks(ctasks << a.lg, FL_THREADS);
            if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_tchunks<T, V>), dim3(cb), dim3(FL_THREADS), 0, st, a, w);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_tchunks<T, 1>), dim3(cb), dim3(FL_THREADS), 0, st, a, w);
        }
        if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_trows<T, V>), dim3(nb), dim3(FL_THREADS), 0, st, a, w, out);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_trows<T, 1>), dim3(nb), dim3(FL_THREADS), 0, st, a, w, out);
    }
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace

size_t feature_count_bytes(int64_t N, int64_t Fin) {
    Carve C{nullptr, 0};
    const int64_t blocks = N * fl_col_blocks(Fin);
    (void)C.take<int32_t>(blocks + 1);
    (void)C.take<int64_t>(1);
    size_t rb = 0;
    (void)rocprim::reduce(nullptr, rb, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(blocks + 1), rocprim::plus<int64_t>(), (hipStream_t)0);
    (void)C.take<char>((int64_t)rb);
    return C.off + 256;
}

int feature_count_run(hipStream_t st, void* ws, size_t ws_bytes, const void* x, int64_t N, int64_t Fin, int flags, int64_t* nnz) {
    if (feature_count_bytes(N, Fin) > ws_bytes) return RLAP_E_WORKSPACE;
    Carve C{static_cast<char*>(ws), 0};
    const int64_t nb = fl_col_blocks(Fin), blocks = N * nb;
    int32_t* cnt = C.take<int32_t>(blocks + 1);
    int64_t* sum = C.take<int64_t>(1);
    size_t rb = 0;
    (void)rocprim::reduce(nullptr, rb, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(blocks + 1), rocprim::plus<int64_t>(), (hipStream_t)0);
    void* tmp = C.take<char>((int64_t)rb);
    const unsigned g = fl_blocks(blocks * 64, FL_THREADS);
    if (flags & RLAP_FEAT_X_F32) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_count_rows<float>), dim3(g), dim3(FL_THREADS), 0, st, static_cast<const float*>(x), N, Fin, nb, cnt);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_fl_count_rows<double>), dim3(g), dim3(FL_THREADS), 0, st, static_cast<const double*>(x), N, Fin, nb, cnt);
    RLAP_HIPCHK(hipGetLastError());
    RLAP_HIPCHK(rocprim::reduce(tmp, rb, cnt, sum, (int64_t)0, (size_t)(blocks + 1), rocprim::plus<int64_t>(), st));
    int64_t h = 0;
    RLAP_HIPCHK(hipMemcpyAsync(&h, sum, 8, hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    *nnz = h;
    return RLAP_OK;
}

size_t feature_build_bytes(int64_t N, int64_t Fin, int flags) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_build(C, N, Fin, flags, B);
}

int feature_build_run(hipStream_t st, void* ws, size_t ws_bytes, const FeatureBuildArgs& g, rlap_feature_desc* desc, FeatureReport* rep) {
    *rep = FeatureReport{};
    const int64_t N = g.N, Fin = g.Fin, nnz = g.nnz;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_build(C, N, Fin, g.flags, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const bool want[2] = {(g.flags & RLAP_PLAN_FORWARD) != 0, (g.flags & RLAP_PLAN_TRANSPOSED) != 0};
    const featlin::Layout L = featlin::layout(N, Fin, nnz, want[0], want[1]);
    if ((size_t)L.bytes > g.plan_bytes) return RLAP_E_BAD_ARG;
    char* pb = static_cast<char*>(g.plan);
    const int64_t slots[2] = {N, Fin};
    const int64_t dcap = plan::dir_cap(nnz);
    RLAP_HIPCHK(hipMemsetAsync(B.cnt, 0, sizeof(unsigned long long) * CNT_WORDS, st));
    for (int d = 0; d < 2; ++d) {
        if (!want[d]) continue;
        int64_t* off = reinterpret_cast<int64_t*>(pb + L.off[d]);
        plan::Record* rec = reinterpret_cast<plan::Record*>(pb + L.rec[d]);
        plan::ChunkRef* dir = reinterpret_cast<plan::ChunkRef*>(pb + L.dir[d]);
        const int rc = (g.flags & RLAP_FEAT_X_F32) ? build_lists<float>(st, static_cast<const float*>(g.x), N, Fin, d, B, off, rec, nnz)
                                                   : build_lists<double>(st, static_cast<const double*>(g.x), N, Fin, d, B, off, rec, nnz);
        if (rc != RLAP_OK) return rc;
        hipLaunchKernelGGL(k_fl_lists, dim3(fl_blocks(slots[d] + 1, 256)), dim3(256), 0, st, off, slots[d], B.nch, B.cnt, d);
        RLAP_HIPCHK(hipGetLastError());
        size_t sb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, sb, B.nch, B.choff[d], (int64_t)0, (size_t)(slots[d] + 1), rocprim::plus<int64_t>(), st));
        if (dcap > 0) {
            hipLaunchKernelGGL(k_fl_dir, dim3(fl_blocks(slots[d], 256)), dim3(256), 0, st, off, slots[d], B.nch, B.choff[d], dir, dcap);
            RLAP_HIPCHK(hipGetLastError());
        }
    }
    // the recounts, the chunk totals and the counters, read back once
    unsigned long long hcnt[CNT_WORDS];
    int64_t hent[2] = {0, 0}, hch[2] = {0, 0};
    RLAP_HIPCHK(hipMemcpyAsync(hcnt, B.cnt, sizeof(hcnt), hipMemcpyDeviceToHost, st));
    for (int d = 0; d < 2; ++d) {
        if (!want[d]) continue;
        RLAP_HIPCHK(hipMemcpyAsync(&hent[d], B.bpos[d] + B.blocks[d], 8, hipMemcpyDeviceToHost, st));
        RLAP_HIPCHK(hipMemcpyAsync(&hch[d], B.choff[d] + slots[d], 8, hipMemcpyDeviceToHost, st));
    }
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs = 1;
    for (int d = 0; d < 2; ++d) {
        if (want[d] && hent[d] != nnz) return RLAP_E_BAD_ARG;   // (the caller's count is not the matrix's: the buffer was sized by it)
    }
    rep->nnz = nnz;
    for (int d = 0; d < 2; ++d) {
        rep->longest[d] = want[d] ? (int64_t)hcnt[d ? CNT_MAX_T : CNT_MAX_F] : -1;
        rep->long_lists[d] = want[d] ? (int64_t)hcnt[d ? CNT_LONG_T : CNT_LONG_F] : -1;
        rep->chunks[d] = want[d] ? hch[d] : -1;
        if (want[d] && (hch[d] < 0 || hch[d] > dcap)) return RLAP_E_INTERNAL;
    }
    *desc = rlap_feature_desc{};
    desc->num_nodes = N; desc->in_features = Fin; desc->nnz = nnz;
    desc->chunks_forward = rep->chunks[0]; desc->chunks_transposed = rep->chunks[1];
    desc->off_forward = L.off[0]; desc->dir_forward = L.dir[0]; desc->rec_forward = L.rec[0];
    desc->off_transposed = L.off[1]; desc->dir_transposed = L.dir[1]; desc->rec_transposed = L.rec[1];
    desc->plan_bytes = L.bytes;
    desc->flags = g.flags;
    desc->magic = featlin::MAGIC;
    return RLAP_OK;
}

size_t feature_apply_bytes(const rlap_feature_desc& d, int64_t K, int64_t Fout, int flags, int64_t part_limit) {
    const int64_t pcap = (flags & RLAP_SPMM_TRANSPOSE) ? part_cap(d.chunks_transposed, K * Fout, part_limit) : 0;
    return (size_t)(plan::align_up(4 * d.in_features) + 8 * pcap * K * Fout + 256);
}

int feature_apply_run(hipStream_t st, void* ws, size_t ws_bytes, const FeatureApplyArgs& g) {
    const rlap_feature_desc& d = *g.desc;
    const bool t = (g.flags & RLAP_SPMM_TRANSPOSE) != 0;
    const char* pb = static_cast<const char*>(g.plan);
    Fu a{};
    a.off = reinterpret_cast<const int64_t*>(pb + (t ? d.off_transposed : d.off_forward));
    a.rec = reinterpret_cast<const plan::Record*>(pb + (t ? d.rec_transposed : d.rec_forward));
    a.dir = reinterpret_cast<const plan::ChunkRef*>(pb + (t ? d.dir_transposed : d.dir_forward));
    a.entries = d.nnz;
    a.chunks = t ? d.chunks_transposed : d.chunks_forward;
    a.N = d.num_nodes; a.Fin = d.in_features; a.F = g.Fout; a.K = (int)g.K;
    a.slots = t ? d.in_features : d.num_nodes;
    a.ids = t ? d.num_nodes : d.in_features;
    a.pcap = t ? part_cap(a.chunks, g.K * g.Fout, g.part_limit) : 0;
    if (feature_apply_bytes(d, g.K, g.Fout, g.flags, g.part_limit) > ws_bytes) return RLAP_E_WORKSPACE;
    a.mask = static_cast<const uint32_t*>(ws);
    a.part = reinterpret_cast<double*>(static_cast<char*>(ws) + plan::align_up(4 * d.in_features));
    return (g.flags & RLAP_SPMM_X_F32) ? launch_sums<float>(st, a, g, t) : launch_sums<double>(st, a, g, t);
}

}  // namespace rlap
