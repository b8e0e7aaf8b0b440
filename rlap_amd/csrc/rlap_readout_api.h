// rlap_readout_api.h -- the per-graph readout (rlap_graph_readout / _backward): the interface between rlap_readout.hip,
// which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.
// The summation rule is rlap_spmm.h's; the work map is in rlap_readout.h.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct ReadoutArgs {
    const void* x; int64_t L, N, F;           // forward: x (L, N, F); backward: gy (L, G, F); float32 with RLAP_READOUT_X_F32
    const int64_t* node_ptr; int64_t G;       // [G+1] on the device
    int flags;                                // RLAP_READOUT_MEAN, RLAP_READOUT_X_F32 (include/rlap_hip.h)
    void* y;                                  // forward: y (L, G, F); backward: gx (L, N, F); of x's type
};

// arena bytes of a forward call (the backward call needs none)
size_t readout_bytes(int64_t L, int64_t N, int64_t F, int64_t G);
// the calls on `stream`; no host synchronisation; return an RLAP_* status
int readout_run(hipStream_t stream, void* ws, size_t ws_bytes, const ReadoutArgs& a);
int readout_backward_run(hipStream_t stream, const ReadoutArgs& a);

}  // namespace rlap
