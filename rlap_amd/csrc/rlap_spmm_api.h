// rlap_spmm_api.h -- GCN propagation of snapshots (rlap_snapshot_propagate): the interface between rlap_spmm.hip, which
// holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.  The
// summation order itself is in rlap_spmm.h.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct SnapshotSpmmArgs {
    SnapshotSeg seg;
    int flags;                                // RLAP_GCN_WEIGHTED / SELF_LOOPS / NORMALIZE, RLAP_SPMM_* (include/rlap_hip.h)
    double fill;                              // weight of an added self loop
    const void* x; int64_t F;                 // (N, F), or with RLAP_SPMM_X_PER_LAYER (S / G, N, F); float32 with RLAP_SPMM_X_F32
    void* y;                                  // (S / G, N, F) of x's type
    int64_t part_limit;                       // test hook: chunk sums the call may keep (negative: the budget of rlap_spmm.hip)
};

struct SnapshotSpmmReport {
    int64_t entries, blocks, chunked_lists;
    int32_t host_syncs;
};

constexpr int64_t SPMM_MAX_F = 65536;                 // feature columns of a call
constexpr int64_t SPMM_MAX_ELEMS = (int64_t)1 << 40;  // elements of the result

// arena bytes of a call
size_t snapshot_spmm_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int64_t F, int flags, int64_t part_limit);
// the call on `stream`, with `ws` (snapshot_spmm_bytes) as its scratch; returns an RLAP_* status
int snapshot_spmm_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotSpmmArgs& a, SnapshotSpmmReport* rep);

}  // namespace rlap
