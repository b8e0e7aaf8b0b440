// rlap_markov_api.h -- Markov diffusion of snapshots (rlap_snapshot_markov): the interface between rlap_markov.hip,
// which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.
#pragma once
#include "rlap_markov.h"
#include "rlap_snapshot.h"

namespace rlap {

struct SnapshotMarkovArgs {
    SnapshotSeg seg;
    double alpha, eps; int32_t order;         // order: D of rlap_markov.h (D + 1 applications of the normalised adjacency)
    int flags;                                // RLAP_MARKOV_* (include/rlap_hip.h)
    double* out; int64_t out_cap;             // (out_cap, 3) rows [i, j, value]
    int64_t* out_ptr;                         // [S+1]
};

struct SnapshotMarkovReport {
    int64_t small_tiles, large_tiles, groups, launches;
    int64_t kept;                             // rows of the output (written, or needed when they exceed out_cap)
    int32_t host_syncs;
};

// arena bytes of a call (an upper bound from the host-known sizes)
size_t snapshot_markov_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int64_t out_cap);
// the call on `stream`, with `ws` (snapshot_markov_bytes) as its scratch; returns an RLAP_* status (RLAP_E_OUT_CAPACITY with
// rep->kept the rows it needs)
int snapshot_markov_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotMarkovArgs& a, SnapshotMarkovReport* rep);

}  // namespace rlap
