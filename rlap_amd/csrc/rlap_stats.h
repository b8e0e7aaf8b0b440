// rlap_stats.h -- snapshot statistics (rlap_snapshot_stats): the interface between rlap_stats.hip, which holds the
// kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rlap {

struct SnapshotStatsArgs {
    const double* sc; int64_t m;              // (m, 3) rows [row, col, w]
    const int64_t* ptr; int64_t S;            // [S+1] segment offsets
    const int64_t* node_ptr; int64_t G;       // [G+1] or nullptr (then G = 1 and every id range is [0, N))
    int64_t N;                                // num_nodes
    int weighted; double tol; int32_t max_iter;
    int64_t* nodes; double* lambda_max; int32_t* iters; int32_t* converged;   // [S] outputs
};

struct SnapshotStatsReport {
    int64_t small_segments, large_segments;
    int64_t lanczos_steps;     // steps of the longest segment
    int64_t large_steps;       // steps enqueued for the large regime (whole chunks; the ones after its last segment stopped are no-ops)
    int64_t large_launches;    // device-wide launches of the large regime
    int32_t host_syncs;
    int32_t not_converged;
};

constexpr int STATS_SMALL_MAX = 7168;     // segments of up to this many nodes run in one workgroup with their vectors in LDS
constexpr int32_t STATS_MAX_ITER = 1024;  // max_iter bound: the tridiagonal of a small segment and its scratch live in LDS too

// The column pass (rlap_stats.hip), shared with the PPR diffusion (rlap_ppr.hip): numbers the blocks of rows that start a new column
// id within a segment over the whole call, checks the layout and maps every row to the block of its row id.  After it, within its
// stream: segment s owns blocks [sb[s], sb[s+1]) and nodes[s] = sb[s+1] - sb[s]; block b is rows [bstart[b], bstart[b+1]); rb[r] is
// the block of row r's id in r's segment (-1 on an error); err[COL_ERR_*] != 0 reports an id out of its range, a column id that
// starts two blocks of one segment, a row id without a column.
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

// arena bytes of a call (an upper bound from the host-known sizes)
size_t snapshot_stats_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int32_t max_iter);
// the call on `stream`, with `ws` (snapshot_stats_bytes) as its scratch; returns an RLAP_* status
int snapshot_stats_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotStatsArgs& a, SnapshotStatsReport* rep);

}  // namespace rlap
