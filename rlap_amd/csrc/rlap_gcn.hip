// rlap_gcn.hip -- encoder-ready snapshots (rlap_snapshot_gcn_norm): for every segment s of a Schur-complement result
// the int64 edge_index, the self loops and the symmetric normalisation coefficients of PyG's gcn_norm,
//     value(i -> j, w) = deg[i]^-1/2 w deg[j]^-1/2,   deg[j] = sum of the weights of the entries whose target (column id) is j,
// in one pass over the rows -- sc[:, :2].long().t().contiguous() + add_remaining_self_loops + scatter + pow + two gathers of every
// view of a call.  A translation unit of its own: no device function is shared with the elimination kernels.
//
//   tables   one workgroup checks ptr / node_ptr and writes the copies every later kernel reads: the tables themselves, or, when they
//            are malformed, well-formed stand-ins ([0, m, m, ...]) with the error word raised -- so nothing has to wait for the host
//            before it may index with them.
//   columns  the column pass (rlap_snapshot.hip): the blocks (one per column id and segment), bstart, rb[r] = block of row r's id,
//            idx[slot of an id] = its block or -1, the layout error words.
//   degrees  16 lanes per block: lane l sums rows l, l + 16, ... of the block into four accumulators in turn (row k of a lane goes to
//            accumulator k % 4), adds them as (a0 + a1) + (a2 + a3), then an xor butterfly over 8, 4, 2, 1 lanes; with self loops the
//            rows i == i stay out of the sum and the loop's weight (that of the block's last loop row, or fill) is added last.  The
//            order depends on nothing but the row's place in its block.  Writes dis[b], the loop weight lw[b]; counts the loop rows.
//   count    only when the input has loop rows and they are to be replaced: loop rows per tile of GCN_TILE rows, then a scan.
//   emit     tiles of GCN_TILE rows staged through LDS with 16-byte loads; row r of segment s goes to entry r - (loop rows in front
//            of r) + (ids of the segments in front of s): three coalesced streams src, dst (8 bytes a lane) and val (4 or 8).
//   eptr     entry offsets of the segments; tail: one lane per id of every range writes its loop behind the segment's rows.
// No atomic touches a floating-point value; the same input gives the same bits.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_gcn.h"
#include "rlap_gcnmath.h"

namespace rlap {
namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_WAVES = GC_THREADS / 64;
constexpr int GC_RPT = GCN_TILE / GC_THREADS;   // rows per thread of an emit tile
constexpr int GC_GROUP = 16;                    // lanes per block of the degree pass
enum { GERR_WEIGHT = GCN_ERR_WEIGHT, GERR_ARG = GCN_ERR_ARG, GERR_WORDS = GCN_ERR_WORDS };

static_assert(GC_RPT * GC_THREADS == GCN_TILE, "an emit tile is a whole number of turns");

// what the kernels share (ptr / node_ptr are the checked copies)
struct Gcn {
    const double* sc; int64_t m;
    const int64_t* ptr; int64_t S;
    const int64_t* node_ptr; int64_t G;
    int64_t N;
    int weighted, loops, normalize;
    double fill;
    const int32_t* rb; const int32_t* blk; const int32_t* bstart; const int32_t* idx; int64_t bcap;
    double* dis; double* lw;                  // [bcap] per block: deg^-1/2 and the weight of the block's loop
    int32_t* cnt; int64_t* tbase; int64_t tiles;   // loop rows per tile, and in front of every tile
    int64_t* segl;                            // [S+1] loop rows in front of a segment's first row
    unsigned long long* tot;                  // [0] loop rows of the call
    int32_t* err;
};

// ids of the segments in front of segment s (s = S: of all segments): the loops written before those of s
__device__ inline int64_t ids_before(const Gcn& a, int64_t s) {
    if (!a.loops) return 0;
    return (s / a.G) * a.N + (a.node_ptr ? a.node_ptr[s % a.G] : 0);
}

__device__ inline double dis_at(const Gcn& a, int32_t b) { return (b >= 0 && b < a.bcap) ? a.dis[b] : 0.0; }

// the offset tables: first entry 0, non-decreasing, last entry the length they index -- copied when they are, replaced by
// [0, len, len, ...] when they are not (GERR_ARG), so that every later kernel indexes with a well-formed table
__global__ __launch_bounds__(1024) void k_gc_tables(const int64_t* __restrict__ ptr, int64_t S, int64_t m, const int64_t* __restrict__ node_ptr,
                                                    int64_t G, int64_t N, int64_t* __restrict__ cptr, int64_t* __restrict__ cnp,
                                                    int32_t* __restrict__ err) {
    __shared__ int bad_p, bad_n;
    const int tid = threadIdx.x;
    if (tid == 0) {
        bad_p = (ptr[0] != 0 || ptr[S] != m) ? 1 : 0;
        bad_n = (node_ptr && (node_ptr[0] != 0 || node_ptr[G] != N)) ? 1 : 0;
    }
    __syncthreads();
    for (int64_t s = tid; s < S; s += blockDim.x) if (ptr[s + 1] < ptr[s]) bad_p = 1;
    if (node_ptr) for (int64_t g = tid; g < G; g += blockDim.x) if (node_ptr[g + 1] < node_ptr[g]) bad_n = 1;
    __syncthreads();
    const int bp = bad_p, bn = bad_n;
    for (int64_t s = tid; s <= S; s += blockDim.x) cptr[s] = bp ? (s == 0 ? 0 : m) : ptr[s];
    if (node_ptr) for (int64_t g = tid; g <= G; g += blockDim.x) cnp[g] = bn ? (g == 0 ? 0 : N) : node_ptr[g];
    if (tid == 0 && (bp || bn)) err[GERR_ARG] = 1;
}

// per block: dis, the loop's weight, the loop rows
__global__ __launch_bounds__(GC_THREADS) void k_gc_degree(Gcn a, int check) {
    const int64_t b = ((int64_t)blockIdx.x * GC_THREADS + threadIdx.x) / GC_GROUP;
    const int sub = threadIdx.x & (GC_GROUP - 1);
    const int64_t nb = std::min<int64_t>(a.blk[a.m - 1], a.bcap);
    if (b >= nb) return;   // (whole groups leave: the butterflies below stay inside a group)
    const int64_t r0 = std::min<int64_t>(std::max<int64_t>(a.bstart[b], 0), a.m);
    const int64_t r1 = std::min<int64_t>(std::max<int64_t>(a.bstart[b + 1], r0), a.m);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int nl = 0;
    int64_t last = -1;
    bool bad = false;
    for (int64_t r = r0 + sub; r < r1; r += 4 * GC_GROUP) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t q = r + u * GC_GROUP;
            if (q < r1) {
                const double vi = a.sc[3 * q], vj = a.sc[3 * q + 1];
                const double w = a.weighted ? a.sc[3 * q + 2] : 1.0;
                if (check && !gcnmath::weight_ok(w)) bad = true;
                if (a.loops && vi == vj) { ++nl; last = q; }
                else acc[u] += w;
            }
        }
    }
    double d = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int o = GC_GROUP / 2; o > 0; o >>= 1) {
        d += __shfl_xor(d, o);
        nl += __shfl_xor(nl, o);
        last = std::max<int64_t>(last, __shfl_xor(last, o));
    }
    if (bad) atomicOr(&a.err[GERR_WEIGHT], 1);
    if (sub != 0) return;
    double w = a.fill;
    if (last >= 0) w = a.weighted ? a.sc[3 * last + 2] : 1.0;
    if (a.loops) d += w;
    a.dis[b] = gcnmath::dis(d);
    a.lw[b] = w;
    if (nl > 0) atomicAdd(a.tot, (unsigned long long)nl);
}

// loop rows per tile; nothing to do for an input without loop rows (every elimination result)
__global__ __launch_bounds__(GC_THREADS) void k_gc_count(Gcn a) {
    if (a.tot[0] == 0) return;
    const int64_t r0 = (int64_t)blockIdx.x * GCN_TILE;
    int c = 0;
#pragma unroll
    for (int k = 0; k < GC_RPT; ++k) {
        const int64_t r = r0 + k * GC_THREADS + threadIdx.x;
        const bool lp = r < a.m && a.sc[3 * r] == a.sc[3 * r + 1];
        c += __syncthreads_count(lp ? 1 : 0);
    }
    if (threadIdx.x == 0) a.cnt[blockIdx.x] = c;
}

// the entries of one tile of GCN_TILE rows.  Row lr of the tile is handled by thread lr % GC_THREADS in its turn lr / GC_THREADS, so
// the tile's rows are visited in (turn, wave, lane) order: their input order.
template <typename V>
__global__ __launch_bounds__(GC_THREADS) void k_gc_emit(Gcn a, int vec, int64_t* __restrict__ src, int64_t* __restrict__ dst,
                                                         V* __restrict__ val) {
    __shared__ __attribute__((aligned(16))) double tile[3 * GCN_TILE];
    __shared__ int32_t wcnt[GC_RPT * GC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * GCN_TILE;
    const int rows = (int)std::min<int64_t>(GCN_TILE, a.m - r0);
    const double* __restrict__ in = a.sc + 3 * r0;
    const int n = 3 * rows;
    if (vec) {   // (the tile starts on a 16-byte boundary when sc does: 24 KiB per tile)
        const double2* __restrict__ s2 = reinterpret_cast<const double2*>(in);
        double2* t2 = reinterpret_cast<double2*>(tile);
        for (int q = tid; q < n / 2; q += GC_THREADS) t2[q] = s2[q];
        if ((n & 1) && tid == 0) tile[n - 1] = in[n - 1];
    } else {
        for (int q = tid; q < n; q += GC_THREADS) tile[q] = in[q];
    }
    const bool drop = a.loops && a.tot[0] != 0;   // loop rows leave the list: the same for every workgroup of the call
    int before[GC_RPT];
#pragma unroll
    for (int k = 0; k < GC_RPT; ++k) before[k] = 0;
    __syncthreads();
    if (drop) {
        int pos[GC_RPT];
#pragma unroll
        for (int k = 0; k < GC_RPT; ++k) {
            const int lr = k * GC_THREADS + tid;
            const bool lp = lr < rows && tile[3 * lr] == tile[3 * lr + 1];
            const unsigned long long mk = __ballot(lp);
            pos[k] = __popcll(mk & (((unsigned long long)1 << lane) - 1));
            if (lane == 0) wcnt[k * GC_WAVES + wave] = __popcll(mk);
        }
        __syncthreads();
        int total = 0;
#pragma unroll
        for (int k = 0; k < GC_RPT; ++k) {
            int p = total + pos[k];   // loop rows of the earlier turns, of the earlier waves of this turn, of the lanes below
            for (int q = 0; q < GC_WAVES; ++q) {
                const int c = wcnt[k * GC_WAVES + q];
                p += q < wave ? c : 0;
                total += c;
            }
            before[k] = p;
        }
    }
    const int64_t lbase = drop ? a.tbase[blockIdx.x] : 0;
    const int64_t s_first = seg_of(a.ptr, a.S, r0);
#pragma unroll
    for (int k = 0; k < GC_RPT; ++k) {
        const int lr = k * GC_THREADS + tid;
        if (lr >= rows) continue;
        const int64_t r = r0 + lr;
        const double vi = tile[3 * lr], vj = tile[3 * lr + 1];
        const double w = a.weighted ? tile[3 * lr + 2] : 1.0;
        const int64_t s = seg_near(a.ptr, a.S, r, s_first);
        const int64_t L = lbase + before[k];
        if (drop) for (int64_t q = s; q >= 0 && a.ptr[q] == r; --q) a.segl[q] = L;   // (first row of s, and of the empty ones before)
        if (drop && vi == vj) continue;
        const int64_t e = r - L + ids_before(a, s);
        double v = w;
        if (a.normalize) v = gcnmath::value(dis_at(a, a.rb[r]), w, dis_at(a, a.blk[r] - 1));
        src[e] = (int64_t)vi;
        dst[e] = (int64_t)vj;
        val[e] = (V)v;
    }
}

// eptr[s] = rows, without the dropped loop rows, and ids in front of segment s
__global__ void k_gc_eptr(Gcn a, int64_t* __restrict__ eptr) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > a.S) return;
    int64_t L = 0;
    if (a.loops && a.tot[0] != 0) L = a.ptr[s] >= a.m ? a.tbase[a.tiles] : a.segl[s];
    eptr[s] = a.ptr[s] - L + ids_before(a, s);
}

// the loops: one lane per (layer, id); the loop of id i of segment s is entry eptr[s + 1] - (hi - i)
template <typename V>
__global__ __launch_bounds__(GC_THREADS) void k_gc_tail(Gcn a, const int64_t* __restrict__ eptr, int64_t* __restrict__ src,
                                                         int64_t* __restrict__ dst, V* __restrict__ val) {
    const int64_t t = (int64_t)blockIdx.x * GC_THREADS + threadIdx.x;
    if (t >= (a.S / a.G) * a.N) return;
    const int64_t layer = t / a.N, i = t - layer * a.N;
    const int64_t g = a.node_ptr ? seg_of(a.node_ptr, a.G, i) : 0;
    const int64_t hi = a.node_ptr ? a.node_ptr[g + 1] : a.N;
    const int64_t e = eptr[layer * a.G + g + 1] - (hi - i);
    const int32_t b = a.m > 0 ? a.idx[t] : -1;
    const bool has = b >= 0 && b < a.bcap;
    const double w = has ? a.lw[b] : a.fill;
    const double d = has ? a.dis[b] : gcnmath::dis(a.fill);
    src[e] = i;
    dst[e] = i;
    val[e] = (V)(a.normalize ? gcnmath::value(d, w, d) : w);
}

struct Bufs {
    ColumnBufs col;
    int64_t *cptr, *cnp, *nodes, *tbase, *segl;
    double *dis, *lw;
    int32_t* cnt;
    unsigned long long* tot;
    void* tmp; size_t tmp_bytes;
    int64_t tiles;
};

size_t carve_gcn(Carve& C, int64_t m, int64_t S, int64_t G, int64_t N, Bufs& B) {
    C.off = column_pass_carve(C.base, C.off, m, S, G, N, GERR_WORDS, &B.col);
    B.tiles = (m + GCN_TILE - 1) / GCN_TILE;
    B.cptr = C.take<int64_t>(S + 1);
    B.cnp = C.take<int64_t>(G + 1);
    B.nodes = C.take<int64_t>(S);
    B.dis = C.take<double>(B.col.bcap);
    B.lw = C.take<double>(B.col.bcap);
    B.cnt = C.take<int32_t>(B.tiles + 1);
    B.tbase = C.take<int64_t>(B.tiles + 1);
    B.segl = C.take<int64_t>(S + 1);
    B.tot = C.take<unsigned long long>(1);
    B.tmp_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, B.tmp_bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(B.tiles + 1),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    B.tmp = C.take<char>((int64_t)B.tmp_bytes);
    return C.off + 256;
}

template <typename V>
int emit_and_tail(hipStream_t st, const Gcn& a, const SnapshotGcnArgs& g) {
    V* val = static_cast<V*>(g.val);
    if (a.m > 0) {
        const int vec = (reinterpret_cast<uintptr_t>(a.sc) & 15) == 0 ? 1 : 0;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gc_emit<V>), dim3((unsigned)a.tiles), dim3(GC_THREADS), 0, st, a, vec, g.src, g.dst, val);
    }
    hipLaunchKernelGGL(k_gc_eptr, dim3(grid_blocks(a.S + 1, 256)), dim3(256), 0, st, a, g.eptr);
    const int64_t ids = (a.S / a.G) * a.N;
    if (a.loops && ids > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_gc_tail<V>), dim3(grid_blocks(ids, GC_THREADS)), dim3(GC_THREADS), 0, st, a, g.eptr, g.src, g.dst, val);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace

int gcn_tables_enqueue(hipStream_t st, const int64_t* ptr, int64_t S, int64_t m, const int64_t* node_ptr, int64_t G, int64_t N,
                       int64_t* cptr, int64_t* cnp, int32_t* err) {
    hipLaunchKernelGGL(k_gc_tables, dim3(1), dim3(1024), 0, st, ptr, S, m, node_ptr, G, N, cptr, cnp, err);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int gcn_degree_enqueue(hipStream_t st, const double* sc, int64_t m, int flags, double fill, const ColumnBufs& col, double* dis,
                       double* lw, unsigned long long* tot) {
    const int weighted = (flags & RLAP_GCN_WEIGHTED) ? 1 : 0, loops = (flags & RLAP_GCN_SELF_LOOPS) ? 1 : 0;
    const int normalize = (flags & RLAP_GCN_NORMALIZE) ? 1 : 0;
    Gcn a{};
    a.sc = sc; a.m = m; a.weighted = weighted; a.loops = loops; a.normalize = normalize; a.fill = fill;
    a.rb = col.rb; a.blk = col.blk; a.bstart = col.bstart; a.idx = col.idx; a.bcap = col.bcap;
    a.dis = dis; a.lw = lw; a.tot = tot; a.err = col.err;
    hipLaunchKernelGGL(k_gc_degree, dim3(grid_blocks(col.bcap * GC_GROUP, GC_THREADS)), dim3(GC_THREADS), 0, st, a, weighted && normalize);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int64_t snapshot_gcn_cap(int64_t m, int64_t S, int64_t G, int64_t N, int flags) {
    return m + ((flags & RLAP_GCN_SELF_LOOPS) ? (S / std::max<int64_t>(G, 1)) * N : 0);
}

size_t snapshot_gcn_bytes(int64_t m, int64_t S, int64_t G, int64_t N) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_gcn(C, m, S, G, N, B);
}

int snapshot_gcn_run(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotGcnArgs& g, SnapshotGcnReport* rep) {
    *rep = SnapshotGcnReport{};
    const SnapshotSeg& in = g.seg;
    const int64_t m = in.m, S = in.S, G = in.G, N = in.N;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_gcn(C, m, S, G, N, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const int weighted = (g.flags & RLAP_GCN_WEIGHTED) ? 1 : 0, loops = (g.flags & RLAP_GCN_SELF_LOOPS) ? 1 : 0;
    const int normalize = (g.flags & RLAP_GCN_NORMALIZE) ? 1 : 0;
    Gcn a{in.sc, m, B.cptr, S, in.node_ptr ? B.cnp : nullptr, G, N, weighted, loops, normalize, g.fill,
          B.col.rb, B.col.blk, B.col.bstart, B.col.idx, B.col.bcap, B.dis, B.lw, B.cnt, B.tbase, B.tiles, B.segl, B.tot, B.col.err};
    // 1. the tables, checked and copied; the column pass on the copies
    RLAP_HIPCHK(hipMemsetAsync(B.col.err, 0, sizeof(int32_t) * GERR_WORDS, st));
    RLAP_HIPCHK(hipMemsetAsync(B.tot, 0, sizeof(unsigned long long), st));
    int trc = gcn_tables_enqueue(st, in.ptr, S, m, in.node_ptr, G, N, B.cptr, B.cnp, B.col.err);
    if (trc != RLAP_OK) return trc;
    if (m > 0) {
        const int rc = column_pass_enqueue(st, in.sc, m, a.ptr, S, a.node_ptr, G, N, B.col, B.nodes);
        if (rc != RLAP_OK) return rc;
    }
    // 2. degrees; 3. the loop rows in front of every tile (zeros without a pass over the rows when the input has none)
    if (m > 0 && (normalize || loops)) {
        trc = gcn_degree_enqueue(st, in.sc, m, g.flags, g.fill, B.col, B.dis, B.lw, B.tot);
        if (trc != RLAP_OK) return trc;
    }
    if (loops) {
        RLAP_HIPCHK(hipMemsetAsync(B.cnt, 0, sizeof(int32_t) * (size_t)(B.tiles + 1), st));
        RLAP_HIPCHK(hipMemsetAsync(B.segl, 0, sizeof(int64_t) * (size_t)(S + 1), st));
        if (m > 0) hipLaunchKernelGGL(k_gc_count, dim3((unsigned)B.tiles), dim3(GC_THREADS), 0, st, a);
        RLAP_HIPCHK(hipGetLastError());
        size_t tb = B.tmp_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.tmp, tb, B.cnt, B.tbase, (int64_t)0, (size_t)(B.tiles + 1), rocprim::plus<int64_t>(), st));
    }
    RLAP_HIPCHK(hipGetLastError());
    // 4. the entries, the offsets, the loops
    const int rc = (g.flags & RLAP_GCN_F32) ? emit_and_tail<float>(st, a, g) : emit_and_tail<double>(st, a, g);
    if (rc != RLAP_OK) return rc;
    // 5. the error words and the loop rows, read back once
    int32_t herr[GERR_WORDS];
    unsigned long long hloops = 0;
    RLAP_HIPCHK(hipMemcpyAsync(herr, B.col.err, sizeof(herr), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipMemcpyAsync(&hloops, B.tot, sizeof(hloops), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs = 1;
    if (herr[GERR_ARG]) return RLAP_E_BAD_ARG;
    if (const int lrc = layout_status(herr)) return lrc;
    if (herr[GERR_WEIGHT]) return RLAP_E_BAD_ARG;
    rep->loops_removed = loops ? (int64_t)hloops : 0;
    rep->entries = snapshot_gcn_cap(m, S, G, N, g.flags) - rep->loops_removed;
    return RLAP_OK;
}

}  // namespace rlap
