// rlap_subgraph.hip -- induced subgraphs and relabelling of snapshots (rlap_snapshot_subgraph): for every segment s of
// an (m, 3) row list, the rows whose two ids both lie in the segment's node set, in their input order, optionally with the ids
// replaced by their rank in the set -- torch.unique + subgraph(relabel_nodes=True) of every snapshot of a call, without a sort.
//
// Ids are dense integers, so a node set is a bitmap and a label is a population count (rlap_bitrank.h).  Bit (layer * N + id) with
// layer = s / G: the G graphs of a batch own disjoint id ranges, so one N-bit row serves the G segments of a layer, and because the
// segments are numbered layer-major, graph fastest, the set bits in ascending order are the ids of segment 0, 1, ..., S-1 in turn:
// one exclusive scan over the words' population counts gives every label, every ids_ptr[s] and the position of every id in d_ids.
//
//   mark    one lane per row (or per list entry): range check, then the id's flag, one byte per bit -- a plain load first, a plain
//           store of 1 only when the flag is down.  Stores only raise flags, so the result does not depend on their order.
//   rank    one lane per word packs 64 flags into the bitmap and counts them, rocPRIM exclusive scan, one lane per word writes its
//           set bits as ids and puts word and scan entry side by side (one gather per test or label), one lane per segment ids_ptr.
//   filter  two streaming passes over tiles of SUB_TILE rows staged through LDS with coalesced loads: (a) keep flags, wave ballots,
//           one count per tile; scan of the tile counts; (b) the flags again, positions from the ballots, kept rows compacted in LDS
//           and written with coalesced stores at the tile's base.  The lane of the first row of a segment writes out_ptr.
// Every kernel is safe on malformed tables and ids (they only raise the error words, read back with the totals in the call's one
// host synchronisation).  The segment search is that of rlap_snapshot.h; no device function is shared with the elimination kernels.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_bitrank.h"
#include "rlap_subgraph.h"

namespace rlap {
namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_WAVES = SG_THREADS / 64;
constexpr int SG_RPT = SUB_TILE / SG_THREADS;   // rows per thread of a filter tile
enum { SERR_ARG = 0, SERR_RANGE = 1, SERR_WORDS = 4 };
enum { TOT_KEPT = 0, TOT_IDS = 1, TOT_WORDS = 2 };

// what the kernels share: the segment description, the lists and the bitmap
struct Sub {
    const double* sc; int64_t m;
    const int64_t* ptr; int64_t S;
    const int64_t* node_ptr; int64_t G;
    int64_t N;
    const int64_t* nodes; const int64_t* nodes_ptr; int64_t nodes_len;
    int relabel, noself;
    uint8_t* flags;               // 64 (W + 1) bytes, one per bit: what the mark pass writes
    uint64_t* words; int64_t W;   // W words and a closing zero word, packed from the flags
    int64_t* scan;                // [W+1] set bits in front of every word
    bitrank::Rank* rank;          // [W+1] (word, scan) side by side: what every kernel behind the scan reads
    int32_t* err;
};

// id range of segment s, clipped to [0, N] (a malformed node_ptr is reported by k_sg_check; nothing may index outside the bitmap)
__device__ inline void seg_range(const Sub& a, int64_t s, int64_t* lo, int64_t* hi) {
    if (!a.node_ptr) { *lo = 0; *hi = a.N; return; }
    const int64_t g = s % a.G;
    *lo = std::min<int64_t>(std::max<int64_t>(a.node_ptr[g], 0), a.N);
    *hi = std::min<int64_t>(std::max<int64_t>(a.node_ptr[g + 1], 0), a.N);
}

__device__ inline bool id_ok(double v, int64_t lo, int64_t hi) { return v >= (double)lo && v < (double)hi; }   // (false for NaN)

// One byte per bit while marking: plain stores of 1 (a racing store writes the same value), behind a plain load so that a flag
// that is already up costs no store.  64-bit atomic ORs straight into the bitmap ran the mark pass at half this rate.
__device__ inline void set_flag(uint8_t* __restrict__ flags, int64_t x) {
    if (!flags[x]) flags[x] = 1;
}

// the three offset tables: first entry 0, non-decreasing, last entry the length they index
__global__ void k_sg_check(Sub a) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (t == 0) {
        bad = a.ptr[0] != 0 || a.ptr[a.S] != a.m;
        if (a.node_ptr) bad = bad || a.node_ptr[0] != 0 || a.node_ptr[a.G] != a.N;
        if (a.nodes_ptr) bad = bad || a.nodes_ptr[0] != 0 || a.nodes_ptr[a.S] != a.nodes_len;
    }
    if (t < a.S) {
        bad = bad || a.ptr[t + 1] < a.ptr[t];
        if (a.nodes_ptr) bad = bad || a.nodes_ptr[t + 1] < a.nodes_ptr[t];
    }
    if (a.node_ptr && t < a.G) bad = bad || a.node_ptr[t + 1] < a.node_ptr[t];
    if (bad) atomicOr(&a.err[SERR_ARG], 1);
}

// nodes == NULL: the ids of every row enter the set of its segment (a row i == i does not, with the self-loop rule)
__global__ __launch_bounds__(SG_THREADS) void k_sg_mark_rows(Sub a) {
    const int64_t r0 = (int64_t)blockIdx.x * SG_THREADS;
    const int64_t r = r0 + threadIdx.x;
    if (r >= a.m) return;
    const int64_t s = seg_near(a.ptr, a.S, r, seg_of(a.ptr, a.S, r0));
    int64_t lo, hi;
    seg_range(a, s, &lo, &hi);
    const double vi = a.sc[3 * r], vj = a.sc[3 * r + 1];
    if (!id_ok(vi, lo, hi) || !id_ok(vj, lo, hi)) return;   // (reported by the filter's first pass)
    const int64_t i = (int64_t)vi, j = (int64_t)vj;
    if (a.noself && i == j) return;
    const int64_t base = (s / a.G) * a.N;
    set_flag(a.flags, base + i);
    if (j == i) return;
    // Rows of one column arrive together and would all find its flag down at once: the row behind a marking row of the same
    // segment with the same column id leaves the flag to that row.
    if (r > a.ptr[s]) {
        const double pi = a.sc[3 * r - 3], pj = a.sc[3 * r - 2];
        if (pj == vj && id_ok(pi, lo, hi) && !(a.noself && pi == pj)) return;
    }
    set_flag(a.flags, base + j);
}

// a list per segment: entry e belongs to the segment whose nodes_ptr range holds it
__global__ __launch_bounds__(SG_THREADS) void k_sg_mark_lists(Sub a) {
    const int64_t e = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
    if (e >= a.nodes_len) return;
    const int64_t s = seg_of(a.nodes_ptr, a.S, e);
    int64_t lo, hi;
    seg_range(a, s, &lo, &hi);
    const int64_t v = a.nodes[e];
    if (v < lo || v >= hi) { atomicOr(&a.err[SERR_RANGE], 1); return; }
    set_flag(a.flags, (s / a.G) * a.N + v);
}

// one list for all segments: every layer takes the whole list (each id lies in the range of exactly one graph)
__global__ __launch_bounds__(SG_THREADS) void k_sg_mark_shared(Sub a, int64_t layers) {
    const int64_t t = (int64_t)blockIdx.x * SG_THREADS + threadIdx.x;
    if (t >= layers * a.nodes_len) return;
    const int64_t layer = t / a.nodes_len, e = t - layer * a.nodes_len;
    const int64_t v = a.nodes[e];
    if (v < 0 || v >= a.N) { atomicOr(&a.err[SERR_RANGE], 1); return; }
    set_flag(a.flags, layer * a.N + v);
}

// the bitmap from the flags, one lane per word, and the words' population counts (the closing word included)
__global__ void k_sg_pack(const uint8_t* __restrict__ flags, int64_t W, uint64_t* __restrict__ words, int32_t* __restrict__ pc) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > W) return;
    const uint64_t* __restrict__ f = reinterpret_cast<const uint64_t*>(flags + 64 * x);
    uint64_t w = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const uint64_t v = f[c];
#pragma unroll
        for (int k = 0; k < 8; ++k) w |= ((v >> (8 * k)) & 1) << (8 * c + k);
    }
    words[x] = w;
    pc[x] = bitrank::popc(w);
}

// d_ids: one lane per word writes its set bits from scan[word] on, and puts word and scan side by side for the passes behind
__global__ void k_sg_ids(Sub a, int64_t* __restrict__ ids, int64_t cap) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x > a.W) return;
    uint64_t w = a.words[x];
    int64_t o = a.scan[x];
    a.rank[x] = bitrank::Rank{w, o};
    while (w) {
        const int64_t b = x * 64 + __builtin_ctzll(w);
        if (o < cap) ids[o] = b % a.N;
        ++o;
        w &= w - 1;
    }
}

// ids_ptr[s]: the set bits in front of the first bit of segment s's range; ids_ptr[S] the total
__global__ void k_sg_idsptr(Sub a, int64_t* __restrict__ ids_ptr) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > a.S) return;
    if (s == a.S) { ids_ptr[s] = a.rank[a.W].scan; return; }
    int64_t lo, hi;
    seg_range(a, s, &lo, &hi);
    ids_ptr[s] = bitrank::before(a.rank, (s / a.G) * a.N + lo);
}

// the filter over one tile of SUB_TILE rows.  PASS 0: cnt[tile] = kept rows (and the rows' range check).  PASS 1: the kept rows,
// relabelled or not, at out + tbase[tile] in input order, and out_ptr[s] where the tile holds the first row of segment s.
// Row lr of the tile is handled by thread lr % SG_THREADS in its turn lr / SG_THREADS, so the tile order is (turn, wave, lane).
template <int PASS>
__global__ __launch_bounds__(SG_THREADS) void k_sg_filter(Sub a, int vec, int32_t* __restrict__ cnt, const int64_t* __restrict__ tbase,
                                                           const int64_t* __restrict__ ids_ptr, double* __restrict__ out,
                                                           int64_t* __restrict__ out_ptr) {
    __shared__ __attribute__((aligned(16))) double tile[3 * SUB_TILE];
    __shared__ int32_t wcnt[SG_RPT * SG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * SUB_TILE;
    const int rows = (int)std::min<int64_t>(SUB_TILE, a.m - r0);
    const double* __restrict__ src = a.sc + 3 * r0;
    const int n = 3 * rows;
    if (vec) {   // (the tile starts on a 16-byte boundary when sc does: 24 KiB per tile)
        const double2* __restrict__ s2 = reinterpret_cast<const double2*>(src);
        double2* t2 = reinterpret_cast<double2*>(tile);
        for (int q = tid; q < n / 2; q += SG_THREADS) t2[q] = s2[q];
        if ((n & 1) && tid == 0) tile[n - 1] = src[n - 1];
    } else {
        for (int q = tid; q < n; q += SG_THREADS) tile[q] = src[q];
    }
    __syncthreads();
    const int64_t s_first = seg_of(a.ptr, a.S, r0);
    double oi[SG_RPT], oj[SG_RPT], ow[SG_RPT];
    int64_t seg[SG_RPT];
    int pos[SG_RPT];
    bool keep[SG_RPT];
#pragma unroll
    for (int k = 0; k < SG_RPT; ++k) {
        const int lr = k * SG_THREADS + tid;
        const bool valid = lr < rows;
        bool kp = false;
        seg[k] = -1;
        if (valid) {
            const double vi = tile[3 * lr], vj = tile[3 * lr + 1];
            const int64_t s = seg_near(a.ptr, a.S, r0 + lr, s_first);
            int64_t lo, hi;
            seg_range(a, s, &lo, &hi);
            seg[k] = s;
            if (!id_ok(vi, lo, hi) || !id_ok(vj, lo, hi)) {
                if (PASS == 0) atomicOr(&a.err[SERR_RANGE], 1);
            } else {
                const int64_t i = (int64_t)vi, j = (int64_t)vj;
                const int64_t base = (s / a.G) * a.N;
                const bitrank::Rank ei = a.rank[(base + i) >> 6], ej = a.rank[(base + j) >> 6];
                kp = !(a.noself && i == j) && bitrank::test(ei, base + i) && bitrank::test(ej, base + j);
                if (PASS == 1 && kp) {
                    oi[k] = vi; oj[k] = vj; ow[k] = tile[3 * lr + 2];
                    if (a.relabel) {
                        const int64_t first = ids_ptr[s];
                        oi[k] = (double)(bitrank::before(ei, base + i) - first);
                        oj[k] = (double)(bitrank::before(ej, base + j) - first);
                    }
                }
            }
        }
        keep[k] = kp;
        const unsigned long long mk = __ballot(kp);
        pos[k] = __popcll(mk & (((unsigned long long)1 << lane) - 1));
        if (lane == 0) wcnt[k * SG_WAVES + wave] = __popcll(mk);
    }
    __syncthreads();   // (every row of the tile is in registers now: pass 1 compacts in place)
    if (PASS == 0) {
        if (tid == 0) {
            int32_t c = 0;
            for (int q = 0; q < SG_RPT * SG_WAVES; ++q) c += wcnt[q];
            cnt[blockIdx.x] = c;
        }
        return;
    }
    const int64_t tb = tbase[blockIdx.x];
    int total = 0;
#pragma unroll
    for (int k = 0; k < SG_RPT; ++k) {
        int p = total + pos[k];   // kept rows of the earlier turns, of the earlier waves of this turn, of the lanes below
        for (int q = 0; q < SG_WAVES; ++q) {
            const int c = wcnt[k * SG_WAVES + q];
            p += q < wave ? c : 0;
            total += c;
        }
        if (seg[k] >= 0) {
            const int64_t r = r0 + k * SG_THREADS + tid;
            for (int64_t s = seg[k]; s >= 0 && a.ptr[s] == r; --s) out_ptr[s] = tb + p;   // (first row of s, and of the empty ones before)
        }
        if (keep[k]) { tile[3 * p] = oi[k]; tile[3 * p + 1] = oj[k]; tile[3 * p + 2] = ow[k]; }
    }
    __syncthreads();
    double* __restrict__ dst = out + 3 * tb;
    for (int q = tid; q < 3 * total; q += SG_THREADS) dst[q] = tile[q];
}

// out_ptr of the segments that start behind the last row, and the totals the host reads
__global__ void k_sg_tail(Sub a, const int64_t* __restrict__ tbase, int64_t tiles, int64_t* __restrict__ out_ptr, int64_t* __restrict__ tot) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s <= a.S && a.ptr[s] >= a.m) out_ptr[s] = tbase[tiles];
    if (s == 0) { tot[TOT_KEPT] = tbase[tiles]; tot[TOT_IDS] = a.rank[a.W].scan; }
}

struct Bufs {
    uint8_t* flags; uint64_t* words; int32_t* pc; int64_t* scan; bitrank::Rank* rank; int32_t* cnt; int64_t* tbase; int32_t* err; int64_t* tot;
    void* tmp; size_t tmp_bytes;
    int64_t W, tiles;
};

static_assert(SG_RPT * SG_THREADS == SUB_TILE, "a filter tile is a whole number of turns");

size_t carve_sub(Carve& C, int64_t m, int64_t S, int64_t G, int64_t N, Bufs& B) {
    B.W = bitrank::words_for((S / std::max<int64_t>(G, 1)) * N);
    B.tiles = (m + SUB_TILE - 1) / SUB_TILE;
    B.flags = C.take<uint8_t>(64 * (B.W + 1));
    B.words = C.take<uint64_t>(B.W + 1);
    B.pc = C.take<int32_t>(B.W + 1);
    B.scan = C.take<int64_t>(B.W + 1);
    B.rank = C.take<bitrank::Rank>(B.W + 1);
    B.cnt = C.take<int32_t>(B.tiles + 1);
    B.tbase = C.take<int64_t>(B.tiles + 1);
    B.err = C.take<int32_t>(SERR_WORDS);
    B.tot = C.take<int64_t>(TOT_WORDS);
    size_t t1 = 0, t2 = 0;
    (void)rocprim::exclusive_scan(nullptr, t1, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(B.W + 1),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    (void)rocprim::exclusive_scan(nullptr, t2, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(B.tiles + 1),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    B.tmp_bytes = std::max(t1, t2);
    B.tmp = C.take<char>((int64_t)B.tmp_bytes);
    return C.off + 256;
}

}  // namespace

int64_t snapshot_subgraph_ids_cap(int64_t m, int64_t S, int64_t G, int64_t N, bool lists, bool per_segment, int64_t nodes_len) {
    const int64_t layers = S / std::max<int64_t>(G, 1);
    if (!lists) return std::min<int64_t>(2 * m, layers * N);
    return per_segment ? nodes_len : layers * nodes_len;
}

size_t snapshot_subgraph_bytes(int64_t m, int64_t S, int64_t G, int64_t N) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_sub(C, m, S, G, N, B);
}

int snapshot_subgraph_run(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotSubArgs& g, SnapshotSubReport* rep) {
    *rep = SnapshotSubReport{};
    const int64_t m = g.seg.m, S = g.seg.S, G = g.seg.G, N = g.seg.N;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_sub(C, m, S, G, N, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const int64_t layers = S / G;
    Sub a{g.seg.sc, m, g.seg.ptr, S, g.seg.node_ptr, G, N, g.nodes, g.nodes_ptr, g.nodes_len, (g.flags & RLAP_SUB_RELABEL) ? 1 : 0,
          (g.flags & RLAP_SUB_NO_SELF_LOOPS) ? 1 : 0, B.flags, B.words, B.W, B.scan, B.rank, B.err};
    // 1. tables checked, flags zeroed and marked
    RLAP_HIPCHK(hipMemsetAsync(B.flags, 0, 64 * (size_t)(B.W + 1), st));
    RLAP_HIPCHK(hipMemsetAsync(B.err, 0, sizeof(int32_t) * SERR_WORDS, st));
    RLAP_HIPCHK(hipMemsetAsync(B.cnt, 0, sizeof(int32_t) * (size_t)(B.tiles + 1), st));
    hipLaunchKernelGGL(k_sg_check, dim3(grid_blocks(std::max(S, G) + 1, 256)), dim3(256), 0, st, a);
    if (!g.nodes) {
        if (m > 0) hipLaunchKernelGGL(k_sg_mark_rows, dim3(grid_blocks(m, SG_THREADS)), dim3(SG_THREADS), 0, st, a);
    } else if (g.nodes_ptr) {
        if (g.nodes_len > 0 && S > 0) hipLaunchKernelGGL(k_sg_mark_lists, dim3(grid_blocks(g.nodes_len, SG_THREADS)), dim3(SG_THREADS), 0, st, a);
    } else if (g.nodes_len > 0 && layers > 0) {
        hipLaunchKernelGGL(k_sg_mark_shared, dim3(grid_blocks(layers * g.nodes_len, SG_THREADS)), dim3(SG_THREADS), 0, st, a, layers);
    }
    RLAP_HIPCHK(hipGetLastError());
    // 2. ranks: the bitmap and its popcounts, their scan, the ids and their offsets
    hipLaunchKernelGGL(k_sg_pack, dim3(grid_blocks(B.W + 1, 256)), dim3(256), 0, st, B.flags, B.W, B.words, B.pc);
    RLAP_HIPCHK(hipGetLastError());
    size_t tb = B.tmp_bytes;
    RLAP_HIPCHK(rocprim::exclusive_scan(B.tmp, tb, B.pc, B.scan, (int64_t)0, (size_t)(B.W + 1), rocprim::plus<int64_t>(), st));
    hipLaunchKernelGGL(k_sg_ids, dim3(grid_blocks(B.W + 1, 256)), dim3(256), 0, st, a, g.ids, g.ids_cap);
    hipLaunchKernelGGL(k_sg_idsptr, dim3(grid_blocks(S + 1, 256)), dim3(256), 0, st, a, g.ids_ptr);
    RLAP_HIPCHK(hipGetLastError());
    // 3. the filter: count per tile, scan, write
    const int vec = (reinterpret_cast<uintptr_t>(g.seg.sc) & 15) == 0 ? 1 : 0;
    if (B.tiles > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sg_filter<0>), dim3((unsigned)B.tiles), dim3(SG_THREADS), 0, st, a, vec, B.cnt, B.tbase, g.ids_ptr,
                           g.out, g.out_ptr);
    RLAP_HIPCHK(hipGetLastError());
    tb = B.tmp_bytes;
    RLAP_HIPCHK(rocprim::exclusive_scan(B.tmp, tb, B.cnt, B.tbase, (int64_t)0, (size_t)(B.tiles + 1), rocprim::plus<int64_t>(), st));
    if (B.tiles > 0)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sg_filter<1>), dim3((unsigned)B.tiles), dim3(SG_THREADS), 0, st, a, vec, B.cnt, B.tbase, g.ids_ptr,
                           g.out, g.out_ptr);
    hipLaunchKernelGGL(k_sg_tail, dim3(grid_blocks(S + 1, 256)), dim3(256), 0, st, a, B.tbase, B.tiles, g.out_ptr, B.tot);
    RLAP_HIPCHK(hipGetLastError());
    // 4. the totals and the error words, read back once
    int64_t htot[TOT_WORDS];
    int32_t herr[SERR_WORDS];
    RLAP_HIPCHK(hipMemcpyAsync(htot, B.tot, sizeof(htot), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipMemcpyAsync(herr, B.err, sizeof(herr), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs = 1;
    if (herr[SERR_ARG]) return RLAP_E_BAD_ARG;
    if (herr[SERR_RANGE]) return RLAP_E_INDEX_RANGE;
    if (htot[TOT_IDS] > g.ids_cap) return RLAP_E_INTERNAL;
    rep->kept = htot[TOT_KEPT];
    rep->ids = htot[TOT_IDS];
    return RLAP_OK;
}

}  // namespace rlap
