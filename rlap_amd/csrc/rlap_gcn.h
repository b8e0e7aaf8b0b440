// rlap_gcn.h -- encoder-ready snapshots (rlap_snapshot_gcn_norm): the interface between rlap_gcn.hip, which holds the
// kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rlap {

struct SnapshotGcnArgs {
    const double* sc; int64_t m;              // (m, 3) rows [row, col, w]
    const int64_t* ptr; int64_t S;            // [S+1] segment offsets
    const int64_t* node_ptr; int64_t G;       // [G+1] or nullptr (then G = 1 and every id range is [0, N))
    int64_t N;                                // num_nodes
    int flags;                                // RLAP_GCN_* (include/rlap_hip.h)
    double fill;                              // weight of an added self loop
    int64_t* src; int64_t* dst; void* val;    // [cap] each; val is float32 with RLAP_GCN_F32, else float64
    int64_t* eptr;                            // [S+1] entry offsets
};

struct SnapshotGcnReport {
    int64_t entries, loops_removed;
    int32_t host_syncs;
};

constexpr int GCN_TILE = 1024;                // rows per workgroup of the emit pass

// entries a call can write (the capacity the caller must give)
int64_t snapshot_gcn_cap(int64_t m, int64_t S, int64_t G, int64_t N, int flags);
// arena bytes of a call
size_t snapshot_gcn_bytes(int64_t m, int64_t S, int64_t G, int64_t N);
// the call on `stream`, with `ws` (snapshot_gcn_bytes) as its scratch; returns an RLAP_* status
int snapshot_gcn_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotGcnArgs& a, SnapshotGcnReport* rep);

}  // namespace rlap
