// rlap_subgraph.h -- induced subgraphs and relabelling of snapshots (rlap_snapshot_subgraph): the interface between
// rlap_subgraph.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock
// and its arena.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct SnapshotSubArgs {
    SnapshotSeg seg;
    const int64_t* nodes;                     // node lists, or nullptr (the set of a segment is the ids of its rows)
    const int64_t* nodes_ptr;                 // [S+1] list offsets, or nullptr (one list for all segments)
    int64_t nodes_len;
    int flags;                                // RLAP_SUB_* (include/rlap_hip.h)
    double* out; int64_t* out_ptr;            // (m, 3) kept rows, [S+1]
    int64_t* ids; int64_t ids_cap;            // sorted distinct ids of every segment's set
    int64_t* ids_ptr;                         // [S+1]
};

struct SnapshotSubReport {
    int64_t kept, ids;                        // rows and ids written
    int32_t host_syncs;
};

constexpr int SUB_TILE = 1024;                // rows per workgroup of the filter passes

// entries of d_ids a call can write (the capacity the caller must give), an upper bound from the host-known sizes
int64_t snapshot_subgraph_ids_cap(int64_t m, int64_t S, int64_t G, int64_t N, bool lists, bool per_segment, int64_t nodes_len);
// arena bytes of a call
size_t snapshot_subgraph_bytes(int64_t m, int64_t S, int64_t G, int64_t N);
// the call on `stream`, with `ws` (snapshot_subgraph_bytes) as its scratch; returns an RLAP_* status
int snapshot_subgraph_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotSubArgs& a, SnapshotSubReport* rep);

}  // namespace rlap
