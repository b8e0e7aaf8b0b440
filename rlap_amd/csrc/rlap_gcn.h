// rlap_gcn.h -- encoder-ready snapshots (rlap_snapshot_gcn_norm): the interface between rlap_gcn.hip, which holds the
// kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct SnapshotGcnArgs {
    SnapshotSeg seg;
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


// The first steps of the call, shared with the propagation (rlap_spmm.hip), which must produce the same coefficients bit for bit.
// Error words behind the column pass's: a weight the normalisation refuses, a malformed ptr / node_ptr.
enum { GCN_ERR_WEIGHT = COL_ERR_WORDS, GCN_ERR_ARG = COL_ERR_WORDS + 1, GCN_ERR_WORDS = 8 };
// checks ptr ([S+1], ending at m) and node_ptr ([G+1] ending at N, or nullptr) on the device and writes the copies every later
// kernel indexes with (well-formed stand-ins and err[GCN_ERR_ARG] when they are malformed)
int gcn_tables_enqueue(hipStream_t stream, const int64_t* ptr, int64_t S, int64_t m, const int64_t* node_ptr, int64_t G, int64_t N,
                       int64_t* cptr, int64_t* cnp, int32_t* err);
// after the column pass (m > 0): dis[b] = deg^-1/2 and lw[b] = the loop's weight of every block b, summed in the fixed order of
// DESIGN 4.10; tot[0] (zeroed by the caller) += the loop rows when flags has RLAP_GCN_SELF_LOOPS; err = col.err
int gcn_degree_enqueue(hipStream_t stream, const double* sc, int64_t m, int flags, double fill, const ColumnBufs& col, double* dis,
                       double* lw, unsigned long long* tot);

}  // namespace rlap
