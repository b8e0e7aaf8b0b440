// rlap_ppr.h -- PPR diffusion of snapshots (rlap_snapshot_ppr): the interface between rlap_ppr.hip, which holds the
// kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.
#pragma once
#include "rlap_ppr_tiles.h"
#include "rlap_snapshot.h"

namespace rlap {

struct SnapshotPprArgs {
    SnapshotSeg seg;
    double alpha, eps; int32_t K;             // K: Chebyshev steps (rlap_cheb.h)
    int flags;                                // RLAP_PPR_* (include/rlap_hip.h)
    double* out; int64_t out_cap;             // (out_cap, 3) rows [i, j, value]
    int64_t* out_ptr;                         // [S+1]
};

struct SnapshotPprReport {
    int64_t small_tiles, large_tiles, groups, launches;
    int64_t kept;                             // rows of the output (written, or needed when they exceed out_cap)
    int32_t host_syncs;
};

// (PPR_TILE, PPR_SMALL_MAX, PPR_TILE_BUDGET and the tile and group table: rlap_ppr_tiles.h)

// arena bytes of a call (an upper bound from the host-known sizes)
size_t snapshot_ppr_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int64_t out_cap, int32_t K);
// the call on `stream`, with `ws` (snapshot_ppr_bytes) as its scratch; returns an RLAP_* status (RLAP_E_OUT_CAPACITY with
// rep->kept the rows it needs)
int snapshot_ppr_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotPprArgs& a, SnapshotPprReport* rep);

}  // namespace rlap
