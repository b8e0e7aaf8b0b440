// rlap_stats.h -- snapshot statistics (rlap_snapshot_stats): the interface between rlap_stats.hip, which holds the
// kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct SnapshotStatsArgs {
    SnapshotSeg seg;
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

// arena bytes of a call (an upper bound from the host-known sizes)
size_t snapshot_stats_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int32_t max_iter);
// the call on `stream`, with `ws` (snapshot_stats_bytes) as its scratch; returns an RLAP_* status
int snapshot_stats_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotStatsArgs& a, SnapshotStatsReport* rep);

}  // namespace rlap
