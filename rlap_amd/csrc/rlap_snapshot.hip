// rlap_snapshot.hip -- the shared layer of the snapshot operations (rlap_snapshot.h): the column pass that the statistics, the PPR
// diffusion, the GCN normalisation and the propagation all start with, and the read-back of the offset tables that the two
// operations with host-side regimes (statistics, PPR) share.  No device function is shared with the elimination kernels.
//
// Layout the kernels rely on (checked, never assumed): the output pass writes survivor i's column as one contiguous block of rows
// (row, i, w) (k_sc_compact: row r belongs to the owner with row_off[i] <= r < row_off[i+1]), so within a segment every column id
// starts exactly one block.  A column id that starts two blocks of one segment is reported (RLAP_E_NOT_GROUPED), as is a row id
// without a column of its own (RLAP_E_NOT_SYMMETRIC) or an id outside the segment's range (RLAP_E_INDEX_RANGE).
//
// Blocks are numbered over the whole call (an inclusive scan of the block-start flags), so segment s owns blocks [sb[s], sb[s+1]).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "rlap_snapshot.h"

namespace rlap {
namespace {

// the index slot of id x in segment s (ids of segment s lie in [node_ptr[g], node_ptr[g+1]), g = s % G; segments s and s' with
// s / G == s' / G cover disjoint ranges, so region s / G of N slots holds all of them); -1 when x is not an id of that range
__device__ inline int64_t id_slot(double x, int64_t s, const int64_t* __restrict__ node_ptr, int64_t G, int64_t N) {
    const int64_t g = s % G;
    const int64_t lo = node_ptr ? node_ptr[g] : 0, hi = node_ptr ? node_ptr[g + 1] : N;
    if (!(x >= (double)lo && x < (double)hi) || x != floor(x)) return -1;
    return (s / G) * N + (int64_t)x;
}

__global__ void k_st_flags(const double* __restrict__ sc, int64_t m, int32_t* __restrict__ f) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    f[r] = (r == 0 || sc[3 * r + 1] != sc[3 * (r - 1) + 1]) ? 1 : 0;
}

__global__ void k_st_segmark(const int64_t* __restrict__ ptr, int64_t S, int32_t* __restrict__ f) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= S) return;
    if (ptr[s] < ptr[s + 1]) f[ptr[s]] = 1;   // (a segment's first row starts a block whatever the row before it holds)
}

__global__ void k_st_index_fill(int32_t* __restrict__ idx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) idx[i] = -1;
}

// block starts: bstart[b] = first row of block b, idx[slot of its column id] = b (a second block of the same id: COL_ERR_GROUP)
__global__ void k_st_blocks(const double* __restrict__ sc, int64_t m, const int32_t* __restrict__ f, const int32_t* __restrict__ blk,
                            const int64_t* __restrict__ ptr, int64_t S, const int64_t* __restrict__ node_ptr, int64_t G, int64_t N,
                            int32_t* __restrict__ idx, int32_t* __restrict__ bstart, int64_t bcap, int32_t* __restrict__ err) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    // (more blocks than ids can be told apart: some id starts two blocks or lies out of range -- reported, nothing written past bcap)
    if (r == 0) { if (blk[m - 1] <= bcap) bstart[blk[m - 1]] = (int32_t)m; else atomicOr(&err[COL_ERR_GROUP], 1); }
    if (!f[r]) return;
    const int32_t b = blk[r] - 1;
    if (b < bcap) bstart[b] = (int32_t)r;
    const int64_t slot = id_slot(sc[3 * r + 1], seg_of(ptr, S, r), node_ptr, G, N);
    if (slot < 0) { atomicOr(&err[COL_ERR_RANGE], 1); return; }
    if (atomicCAS(&idx[slot], -1, b) != -1) atomicOr(&err[COL_ERR_GROUP], 1);
}

// sb[s] = blocks before segment s; nodes[s] = its blocks
__global__ void k_st_segblocks(const int64_t* __restrict__ ptr, int64_t S, const int32_t* __restrict__ blk, int64_t* __restrict__ sb,
                               int64_t* __restrict__ nodes) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s > S) return;
    const int64_t p0 = ptr[s];
    const int64_t b0 = p0 == 0 ? 0 : blk[p0 - 1];
    sb[s] = b0;
    if (s < S) {
        const int64_t p1 = ptr[s + 1];
        nodes[s] = (p1 == 0 ? 0 : blk[p1 - 1]) - b0;
    }
}

// rb[r] = block of row r's id in r's segment
__global__ void k_st_rows(const double* __restrict__ sc, int64_t m, const int64_t* __restrict__ ptr, int64_t S,
                          const int64_t* __restrict__ node_ptr, int64_t G, int64_t N, const int32_t* __restrict__ idx,
                          const int64_t* __restrict__ sb, int32_t* __restrict__ rb, int32_t* __restrict__ err) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const int64_t s = seg_of(ptr, S, r);
    const int64_t slot = id_slot(sc[3 * r], s, node_ptr, G, N);
    int32_t b = -1;
    if (slot < 0) atomicOr(&err[COL_ERR_RANGE], 1);
    else {
        b = idx[slot];
        if (b < sb[s] || b >= sb[s + 1]) { atomicOr(&err[COL_ERR_NOCOL], 1); b = -1; }
    }
    rb[r] = b;
}

}  // namespace

size_t column_pass_carve(char* base, size_t off, int64_t m, int64_t S, int64_t G, int64_t N, int err_words, ColumnBufs* B) {
    Carve C{base, off};
    B->idx_n = (S / G) * N;
    B->bcap = std::min<int64_t>(m, B->idx_n);
    B->rb = C.take<int32_t>(m);   // (the block-start flags first, then rb)
    B->blk = C.take<int32_t>(m);
    B->bstart = C.take<int32_t>(B->bcap + 1);
    B->sb = C.take<int64_t>(S + 1);
    B->idx = C.take<int32_t>(B->idx_n);
    B->err = C.take<int32_t>(std::max<int>(err_words, COL_ERR_WORDS));
    B->scan_bytes = 0;
    (void)rocprim::inclusive_scan(nullptr, B->scan_bytes, (const int32_t*)nullptr, (int32_t*)nullptr, (size_t)std::max<int64_t>(m, 1),
                                  rocprim::plus<int32_t>(), (hipStream_t)0);
    B->scan_tmp = C.take<char>((int64_t)B->scan_bytes);
    return C.off;
}

int column_pass_enqueue(hipStream_t st, const double* sc, int64_t m, const int64_t* ptr, int64_t S, const int64_t* node_ptr, int64_t G,
                        int64_t N, const ColumnBufs& B, int64_t* nodes) {
    int32_t* f = B.rb;   // block-start flags, then (k_st_rows) the row -> block map
    hipLaunchKernelGGL(k_st_flags, dim3(grid_blocks(m, 256)), dim3(256), 0, st, sc, m, f);
    hipLaunchKernelGGL(k_st_segmark, dim3(grid_blocks(S, 256)), dim3(256), 0, st, ptr, S, f);
    hipLaunchKernelGGL(k_st_index_fill, dim3((unsigned)std::min<int64_t>(4096, grid_blocks(B.idx_n, 256))), dim3(256), 0, st, B.idx, B.idx_n);
    RLAP_HIPCHK(hipGetLastError());
    size_t sb_bytes = B.scan_bytes;
    RLAP_HIPCHK(rocprim::inclusive_scan(B.scan_tmp, sb_bytes, f, B.blk, (size_t)m, rocprim::plus<int32_t>(), st));
    hipLaunchKernelGGL(k_st_blocks, dim3(grid_blocks(m, 256)), dim3(256), 0, st, sc, m, f, B.blk, ptr, S, node_ptr, G, N,
                       B.idx, B.bstart, B.bcap, B.err);
    hipLaunchKernelGGL(k_st_segblocks, dim3(grid_blocks(S + 1, 256)), dim3(256), 0, st, ptr, S, B.blk, B.sb, nodes);
    hipLaunchKernelGGL(k_st_rows, dim3(grid_blocks(m, 256)), dim3(256), 0, st, sc, m, ptr, S, node_ptr, G, N, B.idx, B.sb, f, B.err);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int read_tables_checked(hipStream_t st, const int64_t* ptr, int64_t S, int64_t m, const int64_t* node_ptr, int64_t G, int64_t N,
                        std::vector<int64_t>* hptr, std::vector<int64_t>* hnp) {
    hptr->assign((size_t)S + 1, 0);
    hnp->assign((size_t)G + 1, 0);
    RLAP_HIPCHK(hipMemcpyAsync(hptr->data(), ptr, sizeof(int64_t) * (size_t)(S + 1), hipMemcpyDeviceToHost, st));
    if (node_ptr) RLAP_HIPCHK(hipMemcpyAsync(hnp->data(), node_ptr, sizeof(int64_t) * (size_t)(G + 1), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    const auto well_formed = [](const std::vector<int64_t>& t, int64_t last) {
        return t.front() == 0 && t.back() == last && std::is_sorted(t.begin(), t.end());
    };
    if (!well_formed(*hptr, m) || (node_ptr && !well_formed(*hnp, N))) return RLAP_E_BAD_ARG;
    return RLAP_OK;
}

}  // namespace rlap
