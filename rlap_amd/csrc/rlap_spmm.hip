// rlap_spmm.hip -- GCN propagation of snapshots (rlap_snapshot_propagate): y = A^ x (or its transpose) for every layer
// (view x depth) of a Schur-complement result at once, A^ the entry list that rlap_snapshot_gcn_norm produces with the same flags --
// never written out.  A snapshot's rows are grouped by column id and the column id is the target, so an output row is a gather over
// one block of the column pass; the transposed product gets its lists from a stable sort of the rows by the block of their source.
// A translation unit of its own: no device function is shared with the elimination kernels.
//
//   tables   rlap_gcn.hip's: ptr / node_ptr checked on the device, copies (or well-formed stand-ins) for every later kernel.
//   columns  the column pass (rlap_snapshot.hip): blocks, bstart, rb[r] = block of row r's source, idx[slot of an id] = its block.
//   degrees  rlap_gcn.hip's k_gc_degree: dis[b], the loop weight lw[b], the loop rows of the call -- the coefficients are the bits
//            of rlap_snapshot_gcn_norm because they come from the same kernel and the same rlap_gcnmath.h.
//   sources  (transposed only) rocPRIM's stable radix sort of (rb[r], r): perm, and [tlo[b], thi[b]) = the entries whose source is
//            block b's id, in input order.
//   lists    per block: the chunks of its list when it is longer than spmm::CHUNK (0 otherwise), its layer; a scan numbers the
//            chunks of the call.
//   chunks   one group of lanes per (chunk, feature tile) of the long lists: the chunk's sum from 0 in list order, to part[].
//   rows     one group of lanes per (layer, id, feature tile): lanes across the features, 16 bytes a lane where F allows, and
//            64 / ceil_pow2(lanes a row needs) ids per wave when a row needs fewer than 64 lanes.  Four entries' rows of x are
//            loaded before the four dependent adds; the add order is rlap_spmm.h's.  A long list adds its chunk sums in chunk
//            order.  The loop comes last.  Every element of y is written here, 0 for an id without a block and without a loop.
// When the input has loop rows that the flags drop, an entry's place in its list is not its place in its block: the lists of such
// a call are walked by their own group, counting (hand-made inputs only: no elimination result has loop rows).  The same holds for
// the lists whose chunk sums would not fit the part[] budget.  No atomic touches a floating-point value.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_gcn.h"
#include "rlap_gcnmath.h"
#include "rlap_spmm.h"
#include "rlap_spmm_api.h"

namespace rlap {
namespace {

constexpr int SP_THREADS = 256;
constexpr int64_t SP_MAX_GRID = (int64_t)1 << 20;        // workgroups of a launch (the kernels stride over their tasks)
constexpr int64_t SP_PART_BYTES = (int64_t)256 << 20;    // budget of the chunk sums
constexpr int64_t SP_PART_MIN = 4096;                    // chunk sums that always fit
enum { CNT_LOOPS = 0, CNT_CHUNKED = 1, CNT_BLOCKS = 2, CNT_WORDS = 4 };

// (its own grid helper: the cap is applied to the 64-bit count, before it is narrowed)
inline unsigned sp_blocks(int64_t n, int bs) { return capped_blocks(n, bs, SP_MAX_GRID); }

// what the kernels share (ptr is the checked copy)
struct Sp {
    const double* sc; int64_t m;
    const int64_t* ptr; int64_t S, G;
    int64_t N, layers, F;
    int weighted, loops, normalize, transpose, per_layer;
    double fill;
    const int32_t* rb; const int32_t* blk; const int32_t* bstart; const int32_t* idx; int64_t bcap;
    const double* dis; const double* lw;
    unsigned long long* cnt;                  // [CNT_WORDS]
    const int32_t* err;
    int32_t* keys; int32_t* perm; int32_t* tlo; int32_t* thi;   // transposed: sorted blocks, their rows, the range of every block
    int32_t* nch; int32_t* blay; int64_t* choff;                // per block: chunks of a long list, layer; chunks in front
    double* part; int64_t pcap;               // [pcap, F] chunk sums
    int lg; int64_t ftiles;                   // log2 of the lanes of a group; groups a row of F features takes
};

__device__ inline bool sp_failed(const Sp& a) {
    return (a.err[COL_ERR_RANGE] | a.err[COL_ERR_GROUP] | a.err[COL_ERR_NOCOL] | a.err[GCN_ERR_ARG]) != 0;
}

__device__ inline int64_t sp_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the list of block b: n entries from position s on (of the rows, or of perm)
__device__ inline void sp_list(const Sp& a, int64_t b, int64_t& s, int64_t& n) {
    const int64_t lo = a.transpose ? a.tlo[b] : a.bstart[b], hi = a.transpose ? a.thi[b] : a.bstart[b + 1];
    s = sp_clamp(lo, 0, a.m);
    n = sp_clamp(hi, s, a.m) - s;
}

__device__ inline int64_t sp_row(const Sp& a, int64_t s, int64_t k) {
    return a.transpose ? sp_clamp(a.perm[s + k], 0, a.m - 1) : s + k;
}

__device__ inline double sp_dis(const Sp& a, int32_t b) { return (b >= 0 && b < a.bcap) ? a.dis[b] : 0.0; }

// entry r of a list: its coefficient (the value rlap_snapshot_gcn_norm gives row r), the id whose features it takes, and whether
// it is a loop row that left the list
struct SpEntry { double c; int64_t id; bool skip; };
__device__ inline SpEntry sp_entry(const Sp& a, int64_t r, bool drop) {
    const double vi = a.sc[3 * r], vj = a.sc[3 * r + 1];
    const double w = a.weighted ? a.sc[3 * r + 2] : 1.0;
    SpEntry e;
    e.skip = drop && vi == vj;
    e.c = a.normalize ? gcnmath::value(sp_dis(a, a.rb[r]), w, sp_dis(a, a.blk[r] - 1)) : w;
    e.id = sp_clamp((int64_t)(a.transpose ? vj : vi), 0, a.N - 1);
    return e;
}

template <class T, int VEC> __device__ inline void sp_load(const T* __restrict__ p, T (&v)[VEC]) {
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

template <class T, int VEC> __device__ inline void sp_store(T* __restrict__ p, const double (&acc)[VEC]) {
    if constexpr (VEC == 1) {
        p[0] = (T)acc[0];
    } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
    } else {
        *reinterpret_cast<double2*>(p) = make_double2(acc[0], acc[1]);
    }
}

// entries [k0, k1) of the list at s, summed from 0 in list order (none of them a dropped loop row).  Four entries at a time, and
// every stage of the four before the next one -- their rows, then their block indices, then their dis values, then their rows of x --
// so that four loads of each kind are in flight; a turn past the end of the list repeats the last entry's loads (no branch between
// the loads) and keeps the sums as they were, by a select.  The add order is rlap_spmm.h's.
template <class T, int VEC>
__device__ inline void sp_sum_range(const Sp& a, const T* __restrict__ xl, int64_t s, int64_t k0, int64_t k1, int64_t f0, double (&acc)[VEC]) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
    for (int64_t k = k0; k < k1; k += 4) {
        int64_t r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = s + (k + u < k1 ? k + u : k1 - 1);
        if (a.transpose) {   // (one branch around the four loads, not one a load)
            int32_t pr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) pr[u] = a.perm[r[u]];
#pragma unroll
            for (int u = 0; u < 4; ++u) r[u] = pr[u];
        }
        double vi[4], vj[4], w[4];
        int32_t bi[4], bj[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // (every load whatever the flags say: a branch between two loads would make the second wait)
            r[u] = sp_clamp(r[u], 0, a.m - 1);
            vi[u] = a.sc[3 * r[u]];
            vj[u] = a.sc[3 * r[u] + 1];
            w[u] = a.sc[3 * r[u] + 2];
            bi[u] = a.rb[r[u]];
            bj[u] = a.blk[r[u]];
        }
        __builtin_amdgcn_sched_barrier(0);   // (no use of a stage's loads is scheduled between them: the first use would wait for all before it)
        double di[4], dj[4];
        const int32_t bmax = (int32_t)(a.bcap - 1);   // (block numbers are int32; clamped as such, so that nothing is widened beside the loads)
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // (out of range only on a layout error, which the kernels leave on before they come here)
            di[u] = a.dis[(uint32_t)std::min(std::max(bi[u], 0), bmax)];
            dj[u] = a.dis[(uint32_t)std::min(std::max(bj[u] - 1, 0), bmax)];
        }
        __builtin_amdgcn_sched_barrier(0);
        T xv[4][VEC];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t id = sp_clamp((int64_t)(a.transpose ? vj[u] : vi[u]), 0, a.N - 1);
            sp_load<T, VEC>(xl + id * a.F + f0, xv[u]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {   // (a select, not a branch: nothing of an entry can be moved behind a test of its own)
            const bool live = k + u < k1;
            const double wu = a.weighted ? w[u] : 1.0;
            const double cu = a.normalize ? gcnmath::value(di[u], wu, dj[u]) : wu;   // (dis is not read into the result without normalize)
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const double t = spmm::accumulate(acc[v], cu, (double)xv[u][v]);
                acc[v] = live ? t : acc[v];
            }
        }
    }
}

// a whole list by one group, entry by entry: the chunks are counted over the entries that stay.  Returns their number.
template <class T, int VEC>
__device__ inline int64_t sp_sum_counting(const Sp& a, const T* __restrict__ xl, int64_t s, int64_t n, int64_t f0, bool drop, double (&total)[VEC]) {
    double cs[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) { total[v] = 0.0; cs[v] = 0.0; }
    int64_t kept = 0;
    int pos = 0;
    for (int64_t k = 0; k < n; ++k) {
        const SpEntry e = sp_entry(a, sp_row(a, s, k), drop);
        if (e.skip) continue;
        T xv[VEC];
        sp_load<T, VEC>(xl + e.id * a.F + f0, xv);
#pragma unroll
        for (int v = 0; v < VEC; ++v) cs[v] = spmm::accumulate(cs[v], e.c, (double)xv[v]);
        ++kept;
        if (++pos == spmm::CHUNK) {
#pragma unroll
            for (int v = 0; v < VEC; ++v) { total[v] = total[v] + cs[v]; cs[v] = 0.0; }
            pos = 0;
        }
    }
    if (pos > 0) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) total[v] = total[v] + cs[v];
    }
    return kept;
}

__global__ void k_sp_iota(int32_t* __restrict__ v, int64_t m) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += (int64_t)gridDim.x * blockDim.x) v[r] = (int32_t)r;
}

// [tlo[b], thi[b]) = the positions of block b in the sorted keys (both zeroed before: a block without entries as a source)
__global__ void k_sp_bounds(Sp a) {
    if (sp_failed(a)) return;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.m; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t key = a.keys[p];
        if (key < 0 || key >= a.bcap) continue;
        if (p == 0 || a.keys[p - 1] != key) a.tlo[key] = (int32_t)p;
        if (p == a.m - 1 || a.keys[p + 1] != key) a.thi[key] = (int32_t)(p + 1);
    }
}

// per block (and one entry behind the last): the chunks of its list when it is a long one, its layer
__global__ void k_sp_lists(Sp a) {
    const bool ok = !sp_failed(a);
    const int64_t nb = ok ? std::min<int64_t>(a.blk[a.m - 1], a.bcap) : 0;
    const bool drop = a.loops && a.cnt[CNT_LOOPS] != 0;
    for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b <= a.bcap; b += (int64_t)gridDim.x * blockDim.x) {
        int32_t nc = 0;
        if (b < nb) {
            int64_t s, n;
            sp_list(a, b, s, n);
            if (n > spmm::CHUNK && !drop) {   // (with dropped loop rows the walk itself counts the long lists)
                nc = (int32_t)spmm::num_chunks(n);
                atomicAdd(&a.cnt[CNT_CHUNKED], 1ull);
            }
            const int64_t r = sp_clamp(a.bstart[b], 0, a.m - 1);
            a.blay[b] = (int32_t)(seg_of(a.ptr, a.S, r) / a.G);
        }
        a.nch[b] = nc;
        if (b == 0) a.cnt[CNT_BLOCKS] = (unsigned long long)nb;
    }
}

// the chunk sums of the long lists that fit part[]
template <class T, int VEC>
__global__ __launch_bounds__(SP_THREADS) void k_sp_chunks(Sp a, const T* __restrict__ x) {
    if (sp_failed(a) || (a.loops && a.cnt[CNT_LOOPS] != 0)) return;
    const int64_t tasks = std::min<int64_t>(a.choff[a.bcap], a.pcap) * a.ftiles;
    const int64_t lmask = ((int64_t)1 << a.lg) - 1;
    for (int64_t gt = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; (gt >> a.lg) < tasks; gt += (int64_t)gridDim.x * SP_THREADS) {
        const int64_t task = gt >> a.lg;
        const int64_t q = task / a.ftiles, ft = task - q * a.ftiles;
        const int64_t f0 = (((ft << a.lg) | (gt & lmask))) * VEC;
        if (f0 >= a.F) continue;
        int64_t lo = 0, hi = a.bcap;   // the block of chunk q: the last b with choff[b] <= q
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (a.choff[mid] <= q) lo = mid; else hi = mid;
        }
        const int64_t b = lo, k = q - a.choff[b];
        int64_t s, n;
        sp_list(a, b, s, n);
        if (k >= spmm::num_chunks(n)) continue;
        const T* xl = x + (a.per_layer ? (int64_t)a.blay[b] * a.N * a.F : 0);
        double acc[VEC];
        sp_sum_range<T, VEC>(a, xl, s, spmm::chunk_begin(k), spmm::chunk_end(n, k), f0, acc);
#pragma unroll
        for (int v = 0; v < VEC; ++v) a.part[q * a.F + f0 + v] = acc[v];
    }
}

// every element of y
template <class T, int VEC>
__global__ __launch_bounds__(SP_THREADS) void k_sp_rows(Sp a, const T* __restrict__ x, T* __restrict__ y) {
    if (sp_failed(a)) return;
    const int64_t tasks = a.layers * a.N * a.ftiles;
    const int64_t lmask = ((int64_t)1 << a.lg) - 1;
    const bool drop = a.loops && a.m > 0 && a.cnt[CNT_LOOPS] != 0;
    for (int64_t gt = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; (gt >> a.lg) < tasks; gt += (int64_t)gridDim.x * SP_THREADS) {
        const int64_t task = gt >> a.lg;
        const int64_t slot = task / a.ftiles, ft = task - slot * a.ftiles;
        const int64_t f0 = (((ft << a.lg) | (gt & lmask))) * VEC;
        if (f0 >= a.F) continue;
        const int64_t layer = slot / a.N, id = slot - layer * a.N;
        const T* xl = x + (a.per_layer ? layer * a.N * a.F : 0);
        const int32_t b = a.m > 0 ? a.idx[slot] : -1;
        const bool has = b >= 0 && b < a.bcap;
        double total[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) total[v] = 0.0;
        if (has) {
            int64_t s, n;
            sp_list(a, b, s, n);
            const int64_t nc = spmm::num_chunks(n);
            if (drop) {
                const int64_t kept = sp_sum_counting<T, VEC>(a, xl, s, n, f0, true, total);
                if (kept > spmm::CHUNK && f0 == 0) atomicAdd(&a.cnt[CNT_CHUNKED], 1ull);
            } else if (n > spmm::CHUNK && a.choff[b] + nc <= a.pcap) {
                const double* __restrict__ ps = a.part + a.choff[b] * a.F + f0;
                for (int64_t k = 0; k < nc; ++k) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) total[v] = total[v] + ps[k * a.F + v];
                }
            } else {
                for (int64_t k = 0; k < nc; ++k) {
                    double acc[VEC];
                    sp_sum_range<T, VEC>(a, xl, s, spmm::chunk_begin(k), spmm::chunk_end(n, k), f0, acc);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) total[v] = total[v] + acc[v];
                }
            }
        }
        if (a.loops) {   // (the loop of rlap_gcn.hip's k_gc_tail)
            const double w = has ? a.lw[b] : a.fill;
            const double d = has ? a.dis[b] : gcnmath::dis(a.fill);
            const double c = a.normalize ? gcnmath::value(d, w, d) : w;
            T xv[VEC];
            sp_load<T, VEC>(xl + id * a.F + f0, xv);
#pragma unroll
            for (int v = 0; v < VEC; ++v) total[v] = spmm::accumulate(total[v], c, (double)xv[v]);
        }
        sp_store<T, VEC>(y + slot * a.F + f0, total);
    }
}

struct Bufs {
    ColumnBufs col;
    int64_t *cptr, *cnp, *nodes, *choff;
    double *dis, *lw, *part;
    unsigned long long* cnt;
    int32_t *nch, *blay, *keys, *vals, *perm, *tlo, *thi;
    void* scan_tmp; size_t scan_bytes;
    void* sort_tmp; size_t sort_bytes;
    int64_t pcap;
};

// chunk sums the call keeps: every long list's when they fit the budget (a list of n > CHUNK entries has at most 2 n / CHUNK chunks)
int64_t part_cap(int64_t m, int64_t F, int64_t limit) {
    if (m <= spmm::CHUNK) return 0;
    const int64_t worst = 2 * m / spmm::CHUNK + 2;
    if (limit >= 0) return std::min<int64_t>(worst, limit);
    return std::min<int64_t>(worst, std::max<int64_t>(SP_PART_MIN, SP_PART_BYTES / (8 * F)));
}

size_t carve_spmm(Carve& C, int64_t m, int64_t S, int64_t G, int64_t N, int64_t F, int flags, int64_t part_limit, Bufs& B) {
    C.off = column_pass_carve(C.base, C.off, m, S, G, N, GCN_ERR_WORDS, &B.col);
    const int64_t bcap = B.col.bcap;
    B.cptr = C.take<int64_t>(S + 1);
    B.cnp = C.take<int64_t>(G + 1);
    B.nodes = C.take<int64_t>(S);
    B.dis = C.take<double>(bcap);
    B.lw = C.take<double>(bcap);
    B.cnt = C.take<unsigned long long>(CNT_WORDS);
    B.nch = C.take<int32_t>(bcap + 1);
    B.blay = C.take<int32_t>(bcap);
    B.choff = C.take<int64_t>(bcap + 1);
    B.scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, B.scan_bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(bcap + 1),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    B.scan_tmp = C.take<char>((int64_t)B.scan_bytes);
    B.pcap = part_cap(m, F, part_limit);
    B.part = C.take<double>(B.pcap * F);
    B.keys = B.vals = B.perm = B.tlo = B.thi = nullptr;
    B.sort_tmp = nullptr; B.sort_bytes = 0;
    if (flags & RLAP_SPMM_TRANSPOSE) {
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

template <class T>
int launch_sums(hipStream_t st, Sp a, const SnapshotSpmmArgs& g, int64_t pcap) {
    constexpr int V = 16 / (int)sizeof(T);
    const T* x = static_cast<const T*>(g.x);
    T* y = static_cast<T*>(g.y);
    const bool vec = a.F % V == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
    const int64_t lanes = vec ? a.F / V : a.F;   // lanes a row takes
    a.lg = 0;
    while (a.lg < 6 && ((int64_t)1 << a.lg) < lanes) ++a.lg;
    a.ftiles = (lanes + ((int64_t)1 << a.lg) - 1) >> a.lg;
    if (pcap > 0 && a.m > 0) {
        const unsigned nb = sp_blocks((pcap * a.ftiles) << a.lg, SP_THREADS);
        if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sp_chunks<T, V>), dim3(nb), dim3(SP_THREADS), 0, st, a, x);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sp_chunks<T, 1>), dim3(nb), dim3(SP_THREADS), 0, st, a, x);
    }
    const int64_t tasks = a.layers * a.N * a.ftiles;
    if (tasks > 0) {
        const unsigned nb = sp_blocks(tasks << a.lg, SP_THREADS);
        if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sp_rows<T, V>), dim3(nb), dim3(SP_THREADS), 0, st, a, x, y);
        else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sp_rows<T, 1>), dim3(nb), dim3(SP_THREADS), 0, st, a, x, y);
    }
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace

size_t snapshot_spmm_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int64_t F, int flags, int64_t part_limit) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_spmm(C, m, S, G, N, F, flags, part_limit, B);
}

int snapshot_spmm_run(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotSpmmArgs& g, SnapshotSpmmReport* rep) {
    *rep = SnapshotSpmmReport{};
    const SnapshotSeg& in = g.seg;
    const int64_t m = in.m, S = in.S, G = in.G, N = in.N, F = g.F;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_spmm(C, m, S, G, N, F, g.flags, g.part_limit, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const int gflags = g.flags & (RLAP_GCN_WEIGHTED | RLAP_GCN_SELF_LOOPS | RLAP_GCN_NORMALIZE);
    const int loops = (g.flags & RLAP_GCN_SELF_LOOPS) ? 1 : 0, normalize = (g.flags & RLAP_GCN_NORMALIZE) ? 1 : 0;
    const int transpose = (g.flags & RLAP_SPMM_TRANSPOSE) ? 1 : 0;
    Sp a{};
    a.sc = in.sc; a.m = m; a.ptr = B.cptr; a.S = S; a.G = G; a.N = N; a.layers = S / G; a.F = F;
    a.weighted = (g.flags & RLAP_GCN_WEIGHTED) ? 1 : 0; a.loops = loops; a.normalize = normalize; a.transpose = transpose;
    a.per_layer = (g.flags & RLAP_SPMM_X_PER_LAYER) ? 1 : 0;
    a.fill = g.fill;
    a.rb = B.col.rb; a.blk = B.col.blk; a.bstart = B.col.bstart; a.idx = B.col.idx; a.bcap = B.col.bcap;
    a.dis = B.dis; a.lw = B.lw; a.cnt = B.cnt; a.err = B.col.err;
    a.keys = B.keys; a.perm = B.perm; a.tlo = B.tlo; a.thi = B.thi;
    a.nch = B.nch; a.blay = B.blay; a.choff = B.choff; a.part = B.part; a.pcap = B.pcap;
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
        if (transpose) {
            hipLaunchKernelGGL(k_sp_iota, dim3(sp_blocks(m, 256)), dim3(256), 0, st, B.vals, m);
            RLAP_HIPCHK(hipGetLastError());
            size_t sb = B.sort_bytes;
            RLAP_HIPCHK(rocprim::radix_sort_pairs(B.sort_tmp, sb, (const int32_t*)B.col.rb, B.keys, (const int32_t*)B.vals, B.perm, (size_t)m,
                                                0u, 32u, st));
            RLAP_HIPCHK(hipMemsetAsync(B.tlo, 0, sizeof(int32_t) * (size_t)B.col.bcap, st));
            RLAP_HIPCHK(hipMemsetAsync(B.thi, 0, sizeof(int32_t) * (size_t)B.col.bcap, st));
            hipLaunchKernelGGL(k_sp_bounds, dim3(sp_blocks(m, 256)), dim3(256), 0, st, a);
        }
        // 3. the long lists and their chunks
        hipLaunchKernelGGL(k_sp_lists, dim3(sp_blocks(B.col.bcap + 1, 256)), dim3(256), 0, st, a);
        RLAP_HIPCHK(hipGetLastError());
        size_t cb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.nch, B.choff, (int64_t)0, (size_t)(B.col.bcap + 1), rocprim::plus<int64_t>(), st));
    }
    // 4. the sums
    rc = (g.flags & RLAP_SPMM_X_F32) ? launch_sums<float>(st, a, g, B.pcap) : launch_sums<double>(st, a, g, B.pcap);
    if (rc != RLAP_OK) return rc;
    // 5. the error words and the counts, read back once
    int32_t herr[GCN_ERR_WORDS];
    unsigned long long hcnt[CNT_WORDS];
    RLAP_HIPCHK(hipMemcpyAsync(herr, B.col.err, sizeof(herr), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipMemcpyAsync(hcnt, B.cnt, sizeof(hcnt), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs = 1;
    if (herr[GCN_ERR_ARG]) return RLAP_E_BAD_ARG;
    if (const int lrc = layout_status(herr)) return lrc;
    if (herr[GCN_ERR_WEIGHT]) return RLAP_E_BAD_ARG;
    rep->entries = m + (loops ? (S / G) * N - (int64_t)hcnt[CNT_LOOPS] : 0);
    rep->blocks = (int64_t)hcnt[CNT_BLOCKS];
    rep->chunked_lists = (int64_t)hcnt[CNT_CHUNKED];
    return RLAP_OK;
}

}  // namespace rlap
