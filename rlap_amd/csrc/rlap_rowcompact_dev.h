// rlap_rowcompact_dev.h -- what the augmentors that filter the E input rows into K views share (rlap_edgedrop.hip, rlap_nodesample.hip),
// and the small pieces rlap_edgeadd.hip takes of it (the launch macro, clamp, store_row, scan_tmp_bytes).  HIP only; the rules of
// "keep" stay in each user's rule header, which the host mirrors compile without this one.
//
//   compact  the kept rows of every view in input order, two passes over tiles of ROW_TILE rows: pass A (k_rc_count) counts the
//            kept rows per (view, tile), one scan gives the offsets, a one-wave kernel (k_rc_ptr) writes ptr and the row total,
//            pass B (k_rc_write) evaluates the predicate again -- cheaper than a round trip of flags through memory -- and writes
//            [source, target, weight] at offset + rank (ballot and population count within the wave, wave counts in LDS).
//   Pred     a predicate, passed by value.  Row: what a lane remembers of a row over the view loop; row(c, e): that state, for any e
//            (rows past E are never kept, whatever their state); view(k): the per-view constant; keep(k, view, row); MASK: whether
//            pass B also writes Rows::mask -- a compile-time property, so that a user without a mask carries no code for one.
//   lists    per-node lists of rows in input order: the stable radix sort of (key, row number), then [lo, hi) per key and one
//            endpoint gathered into list order (k_rc_bounds).
// k_rc_ptr, k_rc_bounds, list_sort_bytes and build_lists are templates without a parameter of their own: a unit's code object then
// holds only the kernels it launches -- rlap_edgeadd.hip none of these, and not rocPRIM's sort of 32-bit keys either.
// No atomic on a float; LDS holds wave counts only; nothing here waits for the device.
#pragma once
#include <algorithm>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "rlap_edgedrop.h"
#include "rlap_snapshot.h"

// a launch on stream `st` that is counted in `launches`, both of the calling function
#define RLAP_LAUNCH_COUNTED(kernel, grid, block, ...)                                  \
    do {                                                                               \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);       \
        RLAP_HIPCHK(hipGetLastError());                                                \
        ++launches;                                                                    \
    } while (0)

namespace rlap {
namespace rowcompact {

constexpr int ROUNDS = edgedrop::ROW_TILE / edgedrop::TILE;   // rows of a tile a lane owns

__device__ inline int64_t clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ inline void store_row(double* __restrict__ rows, int64_t pos, double s, double d, double w) {
    double* __restrict__ o = rows + 3 * pos;
    o[0] = s; o[1] = d; o[2] = w;
}

// temporary bytes of the int32 -> int64 exclusive scan of `items` counts
inline size_t scan_tmp_bytes(int64_t items) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)items, rocprim::plus<int64_t>(), (hipStream_t)0);
    return bytes;
}

// ---------------------------------------------------------------- compact
struct Rows {
    const int64_t* src; const int64_t* dst; const double* w; int64_t E, nT;   // nT: row tiles
    int K;
    const int32_t* err;                                 // the error word: passes A and B return where it is raised
    int32_t* counts; const int64_t* offs;               // [K * nT + 1], view-major
    double* rows; int64_t cap; int64_t* ptr;
    uint8_t* mask;                                      // [K * E] or null; read by a predicate with MASK only
    int64_t* total;                                     // the row total, for the host's read-back
};

// pass A: the kept rows of every (view, tile)
template <class Pred>
__global__ __launch_bounds__(edgedrop::TILE) void k_rc_count(Rows c, Pred p) {
    constexpr int TILE = edgedrop::TILE, WAVE = edgedrop::WAVE;
    __shared__ int wc[edgedrop::MAX_VIEWS][TILE / WAVE];
    if (*c.err) return;
    const int64_t first = (int64_t)blockIdx.x * edgedrop::ROW_TILE + threadIdx.x;   // the lane's rows: first + r TILE
    typename Pred::Row row[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) row[r] = p.row(c, first + r * TILE);
    for (int k = 0; k < c.K; ++k) {
        const auto view = p.view(k);
        int n = 0;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const bool keep = first + r * TILE < c.E && p.keep(k, view, row[r]);
            n += __popcll(__ballot(keep));
        }
        if ((threadIdx.x & (WAVE - 1)) == 0) wc[k][threadIdx.x / WAVE] = n;
    }
    __syncthreads();
    if ((int)threadIdx.x < c.K) {
        const int k = threadIdx.x;
        c.counts[(int64_t)k * c.nT + blockIdx.x] = (wc[k][0] + wc[k][1]) + (wc[k][2] + wc[k][3]);
    }
}

// ptr[k] = the first row of view k; the total for the host
template <class = void>
__global__ __launch_bounds__(edgedrop::WAVE) void k_rc_ptr(Rows c) {
    const int k = threadIdx.x;
    if (k <= c.K) c.ptr[k] = c.offs[(int64_t)k * c.nT];
    if (k == 0) *c.total = c.offs[(int64_t)c.K * c.nT];
}

// pass B: the predicate again, the rows at offset + rank.  Too little room: no row is written, the mask is.
template <class Pred>
__global__ __launch_bounds__(edgedrop::TILE) void k_rc_write(Rows c, Pred p) {
    constexpr int TILE = edgedrop::TILE, WAVE = edgedrop::WAVE;
    __shared__ int wc[ROUNDS][TILE / WAVE];
    if (*c.err) return;
    const bool fits = c.offs[(int64_t)c.K * c.nT] <= c.cap;
    if (!Pred::MASK && !fits) return;
    const int64_t first = (int64_t)blockIdx.x * edgedrop::ROW_TILE + threadIdx.x;   // the lane's rows: first + r TILE
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    typename Pred::Row row[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) row[r] = p.row(c, first + r * TILE);
    for (int k = 0; k < c.K; ++k) {
        const auto view = p.view(k);
        const int64_t off = c.offs[(int64_t)k * c.nT + blockIdx.x], end = c.offs[(int64_t)k * c.nT + blockIdx.x + 1];
        unsigned kept = 0;
        int rank[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int64_t e = first + r * TILE;
            const bool keep = e < c.E && p.keep(k, view, row[r]);
            const unsigned long long b = __ballot(keep);
            rank[r] = __popcll(b & ((1ull << lane) - 1ull));
            kept |= keep ? 1u << r : 0u;
            if (lane == 0) wc[r][wave] = __popcll(b);
            if (Pred::MASK && c.mask && e < c.E) c.mask[(int64_t)k * c.E + e] = keep ? 1 : 0;
        }
        __syncthreads();
        int pre = 0;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
#pragma unroll
            for (int w = 0; w < TILE / WAVE; ++w) {
                if (w == wave) rank[r] += pre;
                pre += wc[r][w];
            }
        }
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int64_t e = first + r * TILE;
            const int64_t pos = off + rank[r];
            if (!fits || !(kept >> r & 1u) || pos >= end || pos >= c.cap) continue;
            store_row(c.rows, pos, (double)c.src[e], (double)c.dst[e], c.w ? c.w[e] : 1.0);
        }
        __syncthreads();   // (wc is rewritten by the next view)
    }
}

struct Scratch { int32_t* counts; int64_t* offs; void* scan_tmp; size_t scan_bytes; };

inline void carve(Carve& C, int K, int64_t nT, Scratch& S) {
    const int64_t slots = (int64_t)K * nT + 1;
    S.counts = C.take<int32_t>(slots);
    S.offs = C.take<int64_t>(slots);
    S.scan_bytes = scan_tmp_bytes(slots);
    S.scan_tmp = C.take<char>((int64_t)S.scan_bytes);
}

// memset -> count -> scan -> ptr -> write on `st`; passes A and B only where `passes` (a caller without rows or nodes: every count 0)
template <class Pred>
int run(hipStream_t st, const Rows& c, const Pred& p, const Scratch& S, bool passes, int64_t& launches) {
    const size_t slots = (size_t)((int64_t)c.K * c.nT + 1);
    RLAP_HIPCHK(hipMemsetAsync(S.counts, 0, sizeof(int32_t) * slots, st));
    if (passes) RLAP_LAUNCH_COUNTED(k_rc_count<Pred>, (unsigned)c.nT, edgedrop::TILE, c, p);
    size_t cb = S.scan_bytes;
    RLAP_HIPCHK(rocprim::exclusive_scan(S.scan_tmp, cb, S.counts, S.offs, (int64_t)0, slots, rocprim::plus<int64_t>(), st));
    RLAP_LAUNCH_COUNTED(k_rc_ptr<>, 1, edgedrop::WAVE, c);
    if (passes) RLAP_LAUNCH_COUNTED(k_rc_write<Pred>, (unsigned)c.nT, edgedrop::TILE, c, p);
    return RLAP_OK;
}

// ---------------------------------------------------------------- lists
struct Lists {
    int64_t E, N;
    const int32_t* err;
    const uint32_t* key; const int32_t* val;            // [E] a row's key (a node, or any value >= N for none) and its number
    uint32_t* skey; int32_t* perm;                      // [E] both in sorted order
    int32_t* lo; int32_t* hi;                           // [N] the list of node v is [lo[v], hi[v])
    const int64_t* ids; int32_t* out;                   // [E] out[p] = ids[perm[p]], clamped into [0, N)
    void* sort_tmp; size_t sort_bytes;
};

template <class = void>
size_t list_sort_bytes(int64_t E, int64_t N) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr,
                                    (size_t)std::max<int64_t>(E, 1), 0u, edgeplan::key_bits(N), (hipStream_t)0);
    return bytes;
}

// [lo[v], hi[v]) = the positions of key v among the sorted rows (both zeroed before); the ids in list order
template <class = void>
__global__ __launch_bounds__(edgedrop::TILE) void k_rc_bounds(Lists l) {
    constexpr int TILE = edgedrop::TILE;
    if (*l.err) return;
    for (int64_t p = (int64_t)blockIdx.x * TILE + threadIdx.x; p < l.E; p += (int64_t)gridDim.x * TILE) {
        const int64_t key = l.skey[p];
        l.out[p] = (int32_t)clamp(l.ids[clamp(l.perm[p], 0, l.E - 1)], 0, l.N - 1);
        if (key >= l.N) continue;
        if (p == 0 || l.skey[p - 1] != key) l.lo[key] = (int32_t)p;
        if (p == l.E - 1 || l.skey[p + 1] != key) l.hi[key] = (int32_t)(p + 1);
    }
}

// N > 0; with no row every list is empty.  `grid`: the caller's strided grid for E rows.
template <class = void>
int build_lists(hipStream_t st, const Lists& l, unsigned grid, int64_t& launches) {
    RLAP_HIPCHK(hipMemsetAsync(l.lo, 0, sizeof(int32_t) * (size_t)l.N, st));
    RLAP_HIPCHK(hipMemsetAsync(l.hi, 0, sizeof(int32_t) * (size_t)l.N, st));
    if (l.E < 1) return RLAP_OK;
    size_t sb = l.sort_bytes;
    RLAP_HIPCHK(rocprim::radix_sort_pairs(l.sort_tmp, sb, l.key, l.skey, l.val, l.perm, (size_t)l.E, 0u, edgeplan::key_bits(l.N), st));
    RLAP_LAUNCH_COUNTED(k_rc_bounds<>, grid, edgedrop::TILE, l);
    return RLAP_OK;
}

}  // namespace rowcompact
}  // namespace rlap
