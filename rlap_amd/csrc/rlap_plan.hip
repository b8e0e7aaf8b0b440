// rlap_plan.hip -- propagation plans (rlap_snapshot_plan_build / rlap_snapshot_plan_propagate): the x-independent half
// of rlap_snapshot_propagate (rlap_spmm.hip), materialised once into a buffer the caller owns, and the product over it.  A
// translation unit of its own: no device function is shared with the elimination kernels.
//
// The build
//   tables, columns, degrees   as rlap_spmm.hip: rlap_gcn.hip's checked tables, the column pass, k_gc_degree -- so dis[] and lw[]
//            are the very values the unplanned call reads.
//   sources  (transposed) rocPRIM's stable radix sort of (rb[r], r) and the range of every block among the sorted rows, as there.
//   count    per (layer, id) slot and direction: the entries of its list that stay, and the chunks of a long list; with it the
//            loop coefficient of the slot, formed as k_sp_rows forms it.
//   scans    rocPRIM exclusive scans: off[] (int64, in the plan) and the chunk numbering (scratch).
//   fill     the records {coefficient, source id}: forward one lane per row, transposed one lane per sorted position; when the
//            input has loop rows that the flags drop, one lane walks a list, counting (hand-made inputs only).
//   dir      the (slot, chunk) of every chunk number.
//   One read-back of the error words and the counts.
// The planned call
//   chunks   one group of lanes per (chunk number, feature tile): the chunk's sum from 0 in list order, to part[] (arena).
//   rows     one group of lanes per (slot, feature tile), the task shape of k_sp_rows.  Per turn four records (one 16-byte load
//            each, issued back to back), then their four rows of x, then the four adds in list order; a turn past the end of the
//            list repeats the last entry's loads and drops its adds by a select.  A long list adds its chunk sums in chunk order
//            (or, past the part[] budget, sums chunk by chunk itself); the loop term comes last.  Every element of y is written.
// Everything a planned call reads from the plan is clamped before it is used as an index.  No LDS, no atomic on a float.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_gcn.h"
#include "rlap_gcnmath.h"
#include "rlap_plan.h"
#include "rlap_spmm.h"
#include "rlap_spmm_api.h"

namespace rlap {
namespace {

constexpr int PL_THREADS = 256;
constexpr int64_t PL_MAX_GRID = (int64_t)1 << 20;        // workgroups of a launch (the kernels stride over their tasks)
constexpr int64_t PL_PART_BYTES = (int64_t)256 << 20;    // budget of the chunk sums (rlap_spmm.hip's)
constexpr int64_t PL_PART_MIN = 4096;                    // chunk sums that always fit
constexpr int PL_TURN = 4;                               // records of a turn
enum { CNT_LOOPS = 0, CNT_BLOCKS = 1, CNT_CHUNKED_F = 2, CNT_CHUNKED_T = 3, CNT_WORDS = 4 };

inline unsigned pl_blocks(int64_t n, int bs) { return capped_blocks(n, bs, PL_MAX_GRID); }

__device__ inline int64_t pl_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------------------------------------ the build
// what the build's kernels share (ptr is the checked copy)
struct Pb {
    const double* sc; int64_t m;
    const int64_t* ptr; int64_t S, G;
    int64_t N, slots;
    int weighted, loops, normalize;
    double fill;
    const int32_t* rb; const int32_t* blk; const int32_t* bstart; const int32_t* idx; int64_t bcap;
    const double* dis; const double* lw;
    unsigned long long* cnt;                  // [CNT_WORDS]
    const int32_t* err;
    const int32_t* keys; const int32_t* perm; int32_t* tlo; int32_t* thi;   // transposed: sorted blocks, their rows, every block's range
    // one direction
    int transpose;
    int32_t* kept; int32_t* nch;              // [slots + 1] entries that stay, chunks of a long list
    int64_t* off; const int64_t* choff;       // their exclusive scans
    plan::Record* rec; plan::ChunkRef* dir; int64_t dcap;
    double* loopc;                            // [slots] or nullptr (not this launch's to write)
};

__device__ inline bool pb_failed(const Pb& a) {
    return (a.err[COL_ERR_RANGE] | a.err[COL_ERR_GROUP] | a.err[COL_ERR_NOCOL] | a.err[GCN_ERR_ARG]) != 0;
}

// the list of block b: n positions from s on (of the rows, or of perm)
__device__ inline void pb_list(const Pb& a, int64_t b, int64_t& s, int64_t& n) {
    const int64_t lo = a.transpose ? a.tlo[b] : a.bstart[b], hi = a.transpose ? a.thi[b] : a.bstart[b + 1];
    s = pl_clamp(lo, 0, a.m);
    n = pl_clamp(hi, s, a.m) - s;
}

__device__ inline int64_t pb_row(const Pb& a, int64_t s, int64_t k) {
    return a.transpose ? pl_clamp(a.perm[s + k], 0, a.m - 1) : s + k;
}

__device__ inline double pb_dis(const Pb& a, int32_t b) { return (b >= 0 && b < a.bcap) ? a.dis[b] : 0.0; }

// the record of row r: the coefficient rlap_snapshot_gcn_norm gives it, and the id whose features the direction takes
__device__ inline plan::Record pb_record(const Pb& a, int64_t r) {
    const double vi = a.sc[3 * r], vj = a.sc[3 * r + 1];
    const double w = a.weighted ? a.sc[3 * r + 2] : 1.0;
    plan::Record e;
    e.c = a.normalize ? gcnmath::value(pb_dis(a, a.rb[r]), w, pb_dis(a, a.blk[r] - 1)) : w;
    e.id = (int32_t)pl_clamp((int64_t)(a.transpose ? vj : vi), 0, a.N - 1);
    e.zero = 0;
    return e;
}

__device__ inline bool pb_drop(const Pb& a) { return a.loops && a.m > 0 && a.cnt[CNT_LOOPS] != 0; }

__global__ void k_pl_iota(int32_t* __restrict__ v, int64_t m) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (int64_t)gridDim.x * blockDim.x) v[r] = (int32_t)r;
}

// [tlo[b], thi[b]) = the positions of block b in the sorted keys (both zeroed before)
__global__ void k_pl_bounds(Pb a) {
    if (pb_failed(a)) return;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.m; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t key = a.keys[p];
        if (key < 0 || key >= a.bcap) continue;
        if (p == 0 || a.keys[p - 1] != key) a.tlo[key] = (int32_t)p;
        if (p == a.m - 1 || a.keys[p + 1] != key) a.thi[key] = (int32_t)(p + 1);
    }
}

// per slot (and one entry behind the last): the entries of its list that stay, the chunks of a long list; the loop coefficient
__global__ void k_pl_count(Pb a) {
    const bool ok = a.m > 0 && !pb_failed(a);
    const bool drop = pb_drop(a);
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; slot <= a.slots; slot += (int64_t)gridDim.x * blockDim.x) {
        int64_t kept = 0;
        int32_t b = -1;
        if (ok && slot < a.slots) b = a.idx[slot];
        const bool has = b >= 0 && b < a.bcap;
        if (has) {
            int64_t s, n;
            pb_list(a, b, s, n);
            kept = n;
            if (drop) {
                kept = 0;
                for (int64_t k = 0; k < n; ++k) {
                    const int64_t r = pb_row(a, s, k);
                    kept += a.sc[3 * r] == a.sc[3 * r + 1] ? 0 : 1;
                }
            }
        }
        const int64_t nc = plan::dir_chunks(kept);
        if (nc > 0) atomicAdd(&a.cnt[a.transpose ? CNT_CHUNKED_T : CNT_CHUNKED_F], 1ull);
        a.kept[slot] = (int32_t)kept;
        a.nch[slot] = (int32_t)nc;
        if (a.loopc && slot < a.slots) {   // (the loop of rlap_gcn.hip's k_gc_tail, as k_sp_rows forms it)
            const double w = has ? a.lw[b] : a.fill;
            const double d = has ? a.dis[b] : gcnmath::dis(a.fill);
            a.loopc[slot] = a.normalize ? gcnmath::value(d, w, d) : w;
        }
        if (slot == 0) a.cnt[CNT_BLOCKS] = (unsigned long long)(ok ? std::min<int64_t>(a.blk[a.m - 1], a.bcap) : 0);
    }
}

// the records, one lane per row (forward) or per sorted position (transposed); not for an input with dropped loop rows
__global__ void k_pl_fill(Pb a) {
    if (pb_failed(a) || pb_drop(a)) return;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.m; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = a.transpose ? pl_clamp(a.perm[p], 0, a.m - 1) : p;
        const int32_t b = a.transpose ? a.keys[p] : a.blk[r] - 1;   // the block whose list the entry is in
        if (b < 0 || b >= a.bcap) continue;
        const int64_t layer = seg_of(a.ptr, a.S, r) / a.G;
        const int64_t id = pl_clamp((int64_t)(a.transpose ? a.sc[3 * r] : a.sc[3 * r + 1]), 0, a.N - 1);
        const int64_t slot = plan::slot_of(layer, a.N, id);
        const int64_t first = pl_clamp(a.transpose ? a.tlo[b] : a.bstart[b], 0, a.m);
        const int64_t at = plan::record_index(a.off[slot], a.off[slot + 1], plan::place_plain(first, p));
        if (at >= 0 && at < a.m) a.rec[at] = pb_record(a, r);
    }
}

// the records of an input with dropped loop rows: one lane walks a list, counting
__global__ void k_pl_fill_walk(Pb a) {
    if (pb_failed(a) || !pb_drop(a)) return;
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; slot < a.slots; slot += (int64_t)gridDim.x * blockDim.x) {
        const int32_t b = a.idx[slot];
        if (b < 0 || b >= a.bcap) continue;
        int64_t s, n;
        pb_list(a, b, s, n);
        int64_t place = 0;
        for (int64_t k = 0; k < n; ++k) {
            const int64_t r = pb_row(a, s, k);
            if (a.sc[3 * r] == a.sc[3 * r + 1]) continue;
            const int64_t at = plan::record_index(a.off[slot], a.off[slot + 1], place++);
            if (at >= 0 && at < a.m) a.rec[at] = pb_record(a, r);
        }
    }
}

// the directory: the (slot, chunk) of every chunk number
__global__ void k_pl_dir(Pb a) {
    if (pb_failed(a)) return;
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; slot < a.slots; slot += (int64_t)gridDim.x * blockDim.x) {
        if (a.nch[slot] == 0) continue;
        plan::dir_write(slot, a.kept[slot], a.choff[slot], a.dcap, [&](int64_t q, plan::ChunkRef c) { a.dir[q] = c; });
    }
}

struct Bufs {
    ColumnBufs col;
    int64_t *cptr, *cnp, *nodes, *choff[2];
    double *dis, *lw;
    unsigned long long* cnt;
    int32_t *kept, *nch[2], *keys, *vals, *perm, *tlo, *thi;
    void* scan_tmp; size_t scan_bytes;
    void* sort_tmp; size_t sort_bytes;
};

size_t carve_build(Carve& C, int64_t m, int64_t S, int64_t G, int64_t N, int flags, Bufs& B) {
    C.off = column_pass_carve(C.base, C.off, m, S, G, N, GCN_ERR_WORDS, &B.col);
    const int64_t bcap = B.col.bcap, slots = (S / G) * N;
    B.cptr = C.take<int64_t>(S + 1);
    B.cnp = C.take<int64_t>(G + 1);
    B.nodes = C.take<int64_t>(S);
    B.dis = C.take<double>(bcap);
    B.lw = C.take<double>(bcap);
    B.cnt = C.take<unsigned long long>(CNT_WORDS);
    B.kept = C.take<int32_t>(slots + 1);
    for (int d = 0; d < 2; ++d) {
        B.nch[d] = C.take<int32_t>(slots + 1);
        B.choff[d] = C.take<int64_t>(slots + 1);
    }
    B.scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, B.scan_bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(slots + 1),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    B.scan_tmp = C.take<char>((int64_t)B.scan_bytes);
    B.keys = B.vals = B.perm = B.tlo = B.thi = nullptr;
    B.sort_tmp = nullptr; B.sort_bytes = 0;
    if (flags & RLAP_PLAN_TRANSPOSED) {
        B.keys = C.take<int32_t>(m);
        B.vals = C.take<int32_t>(m);
        B.perm = C.take<int32_t>(m);
        B.tlo = C.take<int32_t>(bcap);
        B.thi = C.take<int32_t>(bcap);
        (void)rocprim::radix_sort_pairs(nullptr, B.sort_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr,
                                        (int32_t*)nullptr, (size_t)std::max<int64_t>(m, 1), 0u, 32u, (hipStream_t)0);
        B.sort_tmp = C.take<char>((int64_t)B.sort_bytes);
    }
    return C.off + 256;
}

plan::Layout layout_of(int64_t m, int64_t S, int64_t G, int64_t N, int flags) {
    return plan::layout(m, (S / G) * N, (flags & RLAP_GCN_SELF_LOOPS) != 0, (flags & RLAP_PLAN_FORWARD) != 0,
                        (flags & RLAP_PLAN_TRANSPOSED) != 0);
}

// ------------------------------------------------------------------------------------------------ the planned call
struct Pu {
    const int64_t* off; const plan::Record* rec; const plan::ChunkRef* dir; const double* loopc;
    int64_t entries, chunks;                  // records and directory entries of the direction
    int64_t N, slots, F;
    int per_layer;
    double* part; int64_t pcap;               // [pcap, F] chunk sums
    int lg; int64_t ftiles;                   // log2 of the lanes of a group; groups a row of F features takes
};

template <class T, int VEC> __device__ inline void pl_load(const T* __restrict__ p, T (&v)[VEC]) {
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

template <class T, int VEC> __device__ inline void pl_store(T* __restrict__ p, const double (&acc)[VEC]) {
    if constexpr (VEC == 1) {
        p[0] = (T)acc[0];
    } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    } else {
        *reinterpret_cast<double2*>(p) = make_double2(acc[0], acc[1]);
    }
}

// records [k0, k1) of the list at o0, summed from 0 in list order.  PL_TURN records at a time: their loads back to back, then
// their rows of x back to back, then the adds; a turn past the end repeats the last entry's loads (no branch between the loads)
// and keeps the sums as they were, by a select.  The add order is rlap_spmm.h's.
template <class T, int VEC>
__device__ inline void pl_sum_range(const Pu& a, const T* __restrict__ xl, int64_t o0, int64_t k0, int64_t k1, int64_t f0, double (&acc)[VEC]) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
    const uint4* __restrict__ recs = reinterpret_cast<const uint4*>(a.rec);
    const int32_t nmax = (int32_t)(a.N - 1);
    for (int64_t k = k0; k < k1; k += PL_TURN) {
        uint4 q[PL_TURN];
#pragma unroll
        for (int u = 0; u < PL_TURN; ++u) q[u] = recs[o0 + (k + u < k1 ? k + u : k1 - 1)];
        __builtin_amdgcn_sched_barrier(0);   // (no use of a stage's loads is scheduled between them: the first use would wait for all before it)
        T xv[PL_TURN][VEC];
#pragma unroll
        for (int u = 0; u < PL_TURN; ++u) {
            const int64_t id = (int64_t)std::min(std::max((int32_t)q[u].z, 0), nmax);
            pl_load<T, VEC>(xl + id * a.F + f0, xv[u]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < PL_TURN; ++u) {   // (a select, not a branch: nothing of an entry can be moved behind a test of its own)
            const bool live = k + u < k1;
            const double cu = __hiloint2double((int)q[u].y, (int)q[u].x);
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const double t = spmm::accumulate(acc[v], cu, (double)xv[u][v]);
                acc[v] = live ? t : acc[v];
            }
        }
    }
}

// the list of a slot: n records from o0 on, both clamped to the records the direction has
__device__ inline void pl_list(const Pu& a, int64_t slot, int64_t& o0, int64_t& n) {
    o0 = pl_clamp(a.off[slot], 0, a.entries);
    n = pl_clamp(a.off[slot + 1], o0, a.entries) - o0;
}

// the chunk sums of the long lists that fit part[]
template <class T, int VEC>
__global__ __launch_bounds__(PL_THREADS) void k_pl_chunks(Pu a, const T* __restrict__ x) {
    const int64_t tasks = std::min<int64_t>(a.chunks, a.pcap) * a.ftiles;
    const int64_t lmask = ((int64_t)1 << a.lg) - 1;
    for (int64_t gt = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; (gt >> a.lg) < tasks; gt += (int64_t)gridDim.x * PL_THREADS) {
        const int64_t task = gt >> a.lg;
        const int64_t q = task / a.ftiles, ft = task - q * a.ftiles;
        const int64_t f0 = (((ft << a.lg) | (gt & lmask))) * VEC;
        if (f0 >= a.F) continue;
        const plan::ChunkRef c = a.dir[q];
        const int64_t slot = pl_clamp(c.slot, 0, a.slots - 1);
        int64_t o0, n;
        pl_list(a, slot, o0, n);
        if (c.k < 0 || c.k >= plan::dir_chunks(n)) continue;
        const T* xl = x + (a.per_layer ? (slot / a.N) * a.N * a.F : 0);
        double acc[VEC];
        pl_sum_range<T, VEC>(a, xl, o0, spmm::chunk_begin(c.k), spmm::chunk_end(n, c.k), f0, acc);
#pragma unroll
        for (int v = 0; v < VEC; ++v) a.part[q * a.F + f0 + v] = acc[v];
    }
}

// every element of y
template <class T, int VEC>
__global__ __launch_bounds__(PL_THREADS) void k_pl_rows(Pu a, const T* __restrict__ x, T* __restrict__ y) {
    const int64_t tasks = a.slots * a.ftiles;
    const int64_t lmask = ((int64_t)1 << a.lg) - 1;
    for (int64_t gt = (int64_t)blockIdx.x * PL_THREADS + threadIdx.x; (gt >> a.lg) < tasks; gt += (int64_t)gridDim.x * PL_THREADS) {
        const int64_t task = gt >> a.lg;
        const int64_t slot = task / a.ftiles, ft = task - slot * a.ftiles;
        const int64_t f0 = (((ft << a.lg) | (gt & lmask))) * VEC;
        if (f0 >= a.F) continue;
        const int64_t layer = slot / a.N, id = slot - layer * a.N;
        const T* xl = x + (a.per_layer ? layer * a.N * a.F : 0);
        int64_t o0, n;
        pl_list(a, slot, o0, n);
        double total[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) total[v] = 0.0;
        const int64_t nc = spmm::num_chunks(n);
        int64_t q0 = a.pcap;   // (a short list has no chunk sums: its one chunk is summed here)
        if (n > spmm::CHUNK) q0 = plan::dir_first(a.chunks, slot, [&](int64_t q) { return a.dir[q].slot; });
        if (q0 + nc <= a.pcap) {
            const double* __restrict__ ps = a.part + q0 * a.F + f0;
            for (int64_t k = 0; k < nc; ++k) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) total[v] = total[v] + ps[k * a.F + v];
            }
        } else {
            for (int64_t k = 0; k < nc; ++k) {
                double acc[VEC];
                pl_sum_range<T, VEC>(a, xl, o0, spmm::chunk_begin(k), spmm::chunk_end(n, k), f0, acc);
#pragma unroll
                for (int v = 0; v < VEC; ++v) total[v] = total[v] + acc[v];
            }
        }
        if (a.loopc) {
            const double c = a.loopc[slot];
            T xv[VEC];
            pl_load<T, VEC>(xl + id * a.F + f0, xv);
#pragma unroll
            for (int v = 0; v < VEC; ++v) total[v] = spmm::accumulate(total[v], c, (double)xv[v]);
        }
        pl_store<T, VEC>(y + slot * a.F + f0, total);
    }
}

// chunk sums the call keeps: every chunk of the direction when they fit the budget
int64_t part_cap(int64_t chunks, int64_t F, int64_t limit) {
    if (chunks <= 0) return 0;
    if (limit >= 0) return std::min<int64_t>(chunks, limit);
    return std::min<int64_t>(chunks, std::max<int64_t>(PL_PART_MIN, PL_PART_BYTES / (8 * F)));
}

template <class T>
int launch_sums(hipStream_t st, Pu a, const PlanUseArgs& g) {
    constexpr int V = 16 / (int)sizeof(T);
    const T* x = static_cast<const T*>(g.x);
    T* y = static_cast<T*>(g.y);
    const bool vec = a.F % V == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    const int64_t lanes = vec ? a.F / V : a.F;   // lanes a row takes
    a.lg = 0;
    while (a.lg < 6 && ((int64_t)1 << a.lg) < lanes) ++a.lg;
    a.ftiles = (lanes + ((int64_t)1 << a.lg) - 1) >> a.lg;
    const int64_t ctasks = std::min<int64_t>(a.chunks, a.pcap) * a.ftiles;
    if (ctasks > 0) {   // (no long list, or no chunk sum kept: no chunk kernel)
        const unsigned nb = pl_blocks(ctasks << a.lg, PL_THREADS);
        if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pl_chunks<T, V>), dim3(nb), dim3(PL_THREADS), 0, st, a, x);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pl_chunks<T, 1>), dim3(nb), dim3(PL_THREADS), 0, st, a, x);
    }
    const int64_t tasks = a.slots * a.ftiles;
    if (tasks > 0) {
        const unsigned nb = pl_blocks(tasks << a.lg, PL_THREADS);
        if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pl_rows<T, V>), dim3(nb), dim3(PL_THREADS), 0, st, a, x, y);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pl_rows<T, 1>), dim3(nb), dim3(PL_THREADS), 0, st, a, x, y);
    }
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace

size_t snapshot_plan_buffer_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int flags) {
    return (size_t)layout_of(m, S, G, N, flags).bytes;
}

size_t snapshot_plan_build_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int flags) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_build(C, m, S, G, N, flags, B);
}

int snapshot_plan_build_run(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotPlanArgs& g, rlap_plan_desc* desc,
                            SnapshotPlanReport* rep) {
    *rep = SnapshotPlanReport{};
    const SnapshotSeg& in = g.seg;
    const int64_t m = in.m, S = in.S, G = in.G, N = in.N, slots = (S / G) * N;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_build(C, m, S, G, N, g.flags, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const plan::Layout L = layout_of(m, S, G, N, g.flags);
    if ((size_t)L.bytes > g.plan_bytes) return RLAP_E_BAD_ARG;
    char* pb = static_cast<char*>(g.plan);
    const int gflags = g.flags & (RLAP_GCN_WEIGHTED | RLAP_GCN_SELF_LOOPS | RLAP_GCN_NORMALIZE);
    const int loops = (g.flags & RLAP_GCN_SELF_LOOPS) ? 1 : 0, normalize = (g.flags & RLAP_GCN_NORMALIZE) ? 1 : 0;
    const bool want[2] = {(g.flags & RLAP_PLAN_FORWARD) != 0, (g.flags & RLAP_PLAN_TRANSPOSED) != 0};
    Pb a{};
    a.sc = in.sc; a.m = m; a.ptr = B.cptr; a.S = S; a.G = G; a.N = N; a.slots = slots;
    a.weighted = (g.flags & RLAP_GCN_WEIGHTED) ? 1 : 0; a.loops = loops; a.normalize = normalize;
    a.fill = g.fill;
    a.rb = B.col.rb; a.blk = B.col.blk; a.bstart = B.col.bstart; a.idx = B.col.idx; a.bcap = B.col.bcap;
    a.dis = B.dis; a.lw = B.lw; a.cnt = B.cnt; a.err = B.col.err;
    a.keys = B.keys; a.perm = B.perm; a.tlo = B.tlo; a.thi = B.thi;
    a.kept = B.kept; a.dcap = plan::dir_cap(m);
    // 1. the tables, checked and copied; the column pass on the copies; the degrees of rlap_snapshot_gcn_norm
    RLAP_HIPCHK(hipMemsetAsync(B.col.err, 0, sizeof(int32_t) * GCN_ERR_WORDS, st));
    RLAP_HIPCHK(hipMemsetAsync(B.cnt, 0, sizeof(unsigned long long) * CNT_WORDS, st));
    int rc = gcn_tables_enqueue(st, in.ptr, S, m, in.node_ptr, G, N, B.cptr, B.cnp, B.col.err);
    if (rc != RLAP_OK) return rc;
    if (m > 0) {
        rc = column_pass_enqueue(st, in.sc, m, B.cptr, S, in.node_ptr ? B.cnp : nullptr, G, N, B.col, B.nodes);
        if (rc != RLAP_OK) return rc;
        if (normalize || loops) {
            rc = gcn_degree_enqueue(st, in.sc, m, gflags, g.fill, B.col, B.dis, B.lw, &B.cnt[CNT_LOOPS]);
            if (rc != RLAP_OK) return rc;
        }
        // 2. transposed: the rows of every source, in input order
        if (want[plan::TRANSPOSED]) {
            hipLaunchKernelGGL(k_pl_iota, dim3(pl_blocks(m, 256)), dim3(256), 0, st, B.vals, m);
            RLAP_HIPCHK(hipGetLastError());
            size_t sb = B.sort_bytes;
            RLAP_HIPCHK(rocprim::radix_sort_pairs(B.sort_tmp, sb, (const int32_t*)B.col.rb, B.keys, (const int32_t*)B.vals, B.perm, (size_t)m,
                                                0u, 32u, st));
            RLAP_HIPCHK(hipMemsetAsync(B.tlo, 0, sizeof(int32_t) * (size_t)B.col.bcap, st));
            RLAP_HIPCHK(hipMemsetAsync(B.thi, 0, sizeof(int32_t) * (size_t)B.col.bcap, st));
            hipLaunchKernelGGL(k_pl_bounds, dim3(pl_blocks(m, 256)), dim3(256), 0, st, a);
            RLAP_HIPCHK(hipGetLastError());
        }
    }
    // 3. per direction: counts, scans, records, directory
    bool loop_written = false;
    for (int d = 0; d < 2; ++d) {
        if (!want[d]) continue;
        a.transpose = d;
        a.nch = B.nch[d]; a.choff = B.choff[d];
        a.off = reinterpret_cast<int64_t*>(pb + L.off[d]);
        a.rec = reinterpret_cast<plan::Record*>(pb + L.rec[d]);
        a.dir = reinterpret_cast<plan::ChunkRef*>(pb + L.dir[d]);
        a.loopc = (loops && !loop_written) ? reinterpret_cast<double*>(pb + L.loop) : nullptr;
        loop_written = true;
        hipLaunchKernelGGL(k_pl_count, dim3(pl_blocks(slots + 1, 256)), dim3(256), 0, st, a);
        RLAP_HIPCHK(hipGetLastError());
        size_t cb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.kept, a.off, (int64_t)0, (size_t)(slots + 1), rocprim::plus<int64_t>(), st));
        cb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.nch[d], B.choff[d], (int64_t)0, (size_t)(slots + 1), rocprim::plus<int64_t>(), st));
        if (m > 0) {
            hipLaunchKernelGGL(k_pl_fill, dim3(pl_blocks(m, 256)), dim3(256), 0, st, a);
            if (loops) hipLaunchKernelGGL(k_pl_fill_walk, dim3(pl_blocks(slots, 256)), dim3(256), 0, st, a);
            if (a.dcap > 0) hipLaunchKernelGGL(k_pl_dir, dim3(pl_blocks(slots, 256)), dim3(256), 0, st, a);
            RLAP_HIPCHK(hipGetLastError());
        }
    }
    // 4. the error words and the counts, read back once
    int32_t herr[GCN_ERR_WORDS];
    unsigned long long hcnt[CNT_WORDS];
    int64_t hent[2] = {0, 0}, hch[2] = {0, 0};
    RLAP_HIPCHK(hipMemcpyAsync(herr, B.col.err, sizeof(herr), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipMemcpyAsync(hcnt, B.cnt, sizeof(hcnt), hipMemcpyDeviceToHost, st));
    for (int d = 0; d < 2; ++d) {
        if (!want[d]) continue;
        RLAP_HIPCHK(hipMemcpyAsync(&hent[d], reinterpret_cast<int64_t*>(pb + L.off[d]) + slots, 8, hipMemcpyDeviceToHost, st));
        RLAP_HIPCHK(hipMemcpyAsync(&hch[d], B.choff[d] + slots, 8, hipMemcpyDeviceToHost, st));
    }
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs = 1;
    if (herr[GCN_ERR_ARG]) return RLAP_E_BAD_ARG;
    if (const int lrc = layout_status(herr)) return lrc;
    if (herr[GCN_ERR_WEIGHT]) return RLAP_E_BAD_ARG;
    const int64_t removed = loops ? (int64_t)hcnt[CNT_LOOPS] : 0;
    rep->loops_removed = removed;
    rep->entries = m + (loops ? slots - removed : 0);
    rep->blocks = (int64_t)hcnt[CNT_BLOCKS];
    int64_t used = 256;
    for (int d = 0; d < 2; ++d) {
        rep->dir_entries[d] = want[d] ? hent[d] : -1;
        rep->dir_chunks[d] = want[d] ? hch[d] : -1;
        rep->chunked[d] = want[d] ? (int64_t)hcnt[d ? CNT_CHUNKED_T : CNT_CHUNKED_F] : -1;
        if (!want[d]) continue;
        if (hent[d] < 0 || hent[d] > m || hch[d] < 0 || hch[d] > a.dcap) return RLAP_E_INTERNAL;
        used = std::max<int64_t>(used, L.rec[d] + (int64_t)sizeof(plan::Record) * hent[d]);
        used = std::max<int64_t>(used, L.dir[d] + (int64_t)sizeof(plan::ChunkRef) * a.dcap);
    }
    *desc = rlap_plan_desc{};
    desc->m = m; desc->segments = S; desc->graphs = G; desc->num_nodes = N; desc->fill_value = g.fill;
    desc->entries_forward = rep->dir_entries[0]; desc->entries_transposed = rep->dir_entries[1];
    desc->chunks_forward = rep->dir_chunks[0]; desc->chunks_transposed = rep->dir_chunks[1];
    desc->loop_offset = L.loop;
    desc->off_forward = L.off[0]; desc->dir_forward = L.dir[0]; desc->rec_forward = L.rec[0];
    desc->off_transposed = L.off[1]; desc->dir_transposed = L.dir[1]; desc->rec_transposed = L.rec[1];
    desc->plan_bytes = plan::align_up(used);
    desc->flags = g.flags;
    desc->magic = plan::MAGIC;
    return RLAP_OK;
}

size_t snapshot_plan_use_bytes(const rlap_plan_desc& d, int64_t F, int flags, int64_t part_limit) {
    const int64_t chunks = (flags & RLAP_SPMM_TRANSPOSE) ? d.chunks_transposed : d.chunks_forward;
    return (size_t)(8 * part_cap(chunks, F, part_limit) * F + 256);
}

int snapshot_plan_use_run(hipStream_t st, void* ws, size_t ws_bytes, const PlanUseArgs& g) {
    const rlap_plan_desc& d = *g.desc;
    const int t = (g.flags & RLAP_SPMM_TRANSPOSE) ? 1 : 0;
    const char* pb = static_cast<const char*>(g.plan);
    Pu a{};
    a.off = reinterpret_cast<const int64_t*>(pb + (t ? d.off_transposed : d.off_forward));
    a.rec = reinterpret_cast<const plan::Record*>(pb + (t ? d.rec_transposed : d.rec_forward));
    a.dir = reinterpret_cast<const plan::ChunkRef*>(pb + (t ? d.dir_transposed : d.dir_forward));
    a.loopc = (d.flags & RLAP_GCN_SELF_LOOPS) ? reinterpret_cast<const double*>(pb + d.loop_offset) : nullptr;
    a.entries = t ? d.entries_transposed : d.entries_forward;
    a.chunks = t ? d.chunks_transposed : d.chunks_forward;
    a.N = d.num_nodes; a.slots = (d.segments / d.graphs) * d.num_nodes; a.F = g.F;
    a.per_layer = (g.flags & RLAP_SPMM_X_PER_LAYER) ? 1 : 0;
    a.pcap = part_cap(a.chunks, g.F, g.part_limit);
    if ((size_t)(8 * a.pcap * g.F + 256) > ws_bytes) return RLAP_E_WORKSPACE;
    a.part = static_cast<double*>(ws);
    return (g.flags & RLAP_SPMM_X_F32) ? launch_sums<float>(st, a, g) : launch_sums<double>(st, a, g);
}

}  // namespace rlap
