// rlap_bt_api.h -- the fused Barlow Twins loss (rlap_bt_loss / rlap_bt_loss_backward): the interface between
// rlap_bt.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and
// its arena.  The rule is rlap_bt.h's.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct BtArgs {
    const float* a; const float* b; int64_t N, F;   // the two views' embeddings, (N, F) float32 on the device
    double lambd, eps; int flags;
    // forward: results
    double* terms; double* colstat; float* cross;   // 3 doubles: loss, on, off; 4 F doubles: mean1, sd1, mean2, sd2; F F floats: c
    // backward: the forward's column statistics and cross-correlation, the upstream scalar on the device; results (N, F) each
    const double* colstat_in; const float* cross_in; const double* g; float* ga; float* gb;
};

// arena bytes of the two calls
size_t bt_bytes(int64_t N, int64_t F);
size_t bt_backward_bytes(int64_t N, int64_t F);
// the calls on `stream`; no host synchronisation; return an RLAP_* status
int bt_run(hipStream_t stream, void* ws, size_t ws_bytes, const BtArgs& a);
int bt_backward_run(hipStream_t stream, void* ws, size_t ws_bytes, const BtArgs& a);

}  // namespace rlap
