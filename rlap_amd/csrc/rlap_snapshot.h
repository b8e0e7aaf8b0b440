// rlap_snapshot.h -- what the five snapshot operations (rlap_snapshot_stats / _ppr / _subgraph / _gcn_norm / _propagate, DESIGN
// 4.7-4.11) have in common, once: the HIP check, the arena carver, the grid helper, the segment search, the column pass and the
// host-side checks around it.  The column pass and the table read-back are implemented in rlap_snapshot.hip.
#pragma once
#include <algorithm>
#include <cstdio>
#include <vector>

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/rlap_hip.h"

#define RLAP_HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { std::fprintf(stderr, "[rlap_hip] %s failed: %s (%s:%d)\n", #x, hipGetErrorString(_e), __FILE__, __LINE__); return RLAP_E_HIP; } } while (0)

namespace rlap {

// what every snapshot call starts with: the rows, their segments and the id ranges
struct SnapshotSeg {
    const double* sc; int64_t m;              // (m, 3) rows [row, col, w]
    const int64_t* ptr; int64_t S;            // [S+1] segment offsets
    const int64_t* node_ptr; int64_t G;       // [G+1] or nullptr (then G = 1 and every id range is [0, N))
    int64_t N;                                // num_nodes
};

// pieces of one arena, 256-byte aligned; a null base gives the sizes only, a negative count takes nothing
struct Carve {
    char* base; size_t off;
    template <class T> T* take(int64_t count) {
        off = (off + 255) & ~(size_t)255;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += sizeof(T) * (size_t)(count > 0 ? count : 0);
        return p;
    }
};

inline unsigned grid_blocks(int64_t n, int bs) { return (unsigned)std::max<int64_t>(1, (n + bs - 1) / bs); }
// the same, at most max_grid workgroups: for kernels that stride over their items
inline unsigned capped_blocks(int64_t n, int per_block, int64_t max_grid) { return (unsigned)std::min<int64_t>(max_grid, grid_blocks(n, per_block)); }

// last s in [0, S) with tab[s] <= r (S >= 1): the segment of row r; equal offsets (empty segments) are skipped
__device__ inline int64_t seg_of(const int64_t* __restrict__ tab, int64_t S, int64_t r) {
    int64_t lo = 0, hi = S;   // tab[lo] <= r < tab[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (tab[mid] <= r) lo = mid; else hi = mid;
    }
    return lo;
}

// the segment of row r given that of an earlier row of the same workgroup (rows of a workgroup mostly share one)
__device__ inline int64_t seg_near(const int64_t* __restrict__ tab, int64_t S, int64_t r, int64_t s0) {
    return r < tab[s0 + 1] ? s0 : seg_of(tab, S, r);
}

// The column pass: numbers the blocks of rows that start a new column id within a segment over the whole call, checks the layout
// and maps every row to the block of its row id.  After it, within its stream: segment s owns blocks [sb[s], sb[s+1]) and
// nodes[s] = sb[s+1] - sb[s]; block b is rows [bstart[b], bstart[b+1]); rb[r] is the block of row r's id in r's segment (-1 on an
// error); err[COL_ERR_*] != 0 reports an id out of its range, a column id that starts two blocks of one segment, a row id without
// a column.
enum { COL_ERR_RANGE = 0, COL_ERR_GROUP = 1, COL_ERR_NOCOL = 2, COL_ERR_WORDS = 3 };
struct ColumnBufs {
    int32_t* rb; int32_t* blk; int32_t* bstart; int64_t* sb; int32_t* idx; int32_t* err;
    void* scan_tmp; size_t scan_bytes;
    int64_t bcap, idx_n;       // blocks the tables can hold; id slots
};
// carves the column pass's buffers from `base` (nullptr: sizes only) from offset `off` on; err gets `err_words` >= COL_ERR_WORDS
// words; returns the offset after them
size_t column_pass_carve(char* base, size_t off, int64_t m, int64_t S, int64_t G, int64_t N, int err_words, ColumnBufs* B);
// enqueues the column pass on `stream` (m > 0; the caller has zeroed err)
int column_pass_enqueue(hipStream_t stream, const double* sc, int64_t m, const int64_t* ptr, int64_t S, const int64_t* node_ptr, int64_t G,
                        int64_t N, const ColumnBufs& B, int64_t* nodes);

// the status of the column pass's error words, read back: the first of them that is raised, or RLAP_OK
inline int layout_status(const int32_t* herr) {
    if (herr[COL_ERR_RANGE]) return RLAP_E_INDEX_RANGE;
    if (herr[COL_ERR_GROUP]) return RLAP_E_NOT_GROUPED;
    if (herr[COL_ERR_NOCOL]) return RLAP_E_NOT_SYMMETRIC;
    return RLAP_OK;
}

// copies ptr ([S+1]) and node_ptr ([G+1], or nullptr: hnp stays zero) to the host with one synchronisation of `stream` and checks
// them: first entry 0, non-decreasing, last entry m / N (RLAP_E_BAD_ARG otherwise)
int read_tables_checked(hipStream_t stream, const int64_t* ptr, int64_t S, int64_t m, const int64_t* node_ptr, int64_t G, int64_t N,
                        std::vector<int64_t>* hptr, std::vector<int64_t>* hnp);

}  // namespace rlap
