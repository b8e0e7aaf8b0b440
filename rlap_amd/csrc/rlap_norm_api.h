// rlap_norm_api.h -- the per-view batch norm (rlap_batch_norm / _backward): the interface between rlap_norm.hip, which
// holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and its arena.  The
// rule and the work map are in rlap_norm.h.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct NormArgs {
    const float* x; int64_t L, N, F;          // (L, N, F)
    const float* gy;                          // backward: the upstream gradient (L, N, F)
    const float* weight; const float* bias;   // (F) or null: 1 and 0
    const float* slope;                       // one value, or (F) with RLAP_NORM_SLOPE_PER_CHANNEL; null without PReLU
    const float* running_mean; const float* running_var;   // (F): read in evaluation mode
    float* upd_mean; float* upd_var;          // (F) or null: updated by the training forward call
    double momentum, eps;
    int flags;                                // RLAP_NORM_* (include/rlap_hip.h)
    float* out;                               // forward: y; backward: gx; (L, N, F)
    double* stat;                             // (L, 3, F) c | m | rstd: written by the training forward call, read by its backward call
    float* gweight; float* gbias; float* gslope;   // backward: (F), (F), (1) or (F); null ones are skipped
};

struct NormReport { int vec; int64_t chunks; int launches; };

// arena bytes of a call
size_t norm_bytes(const NormArgs& a, bool backward);
// the calls on `stream`; no host synchronisation; return an RLAP_* status
int norm_run(hipStream_t stream, void* ws, size_t ws_bytes, const NormArgs& a, NormReport* rep);
int norm_backward_run(hipStream_t stream, void* ws, size_t ws_bytes, const NormArgs& a, NormReport* rep);

}  // namespace rlap
