// rlap_rowops_api.h -- the fused bias, activation and dropout pass and the per-row layer norm (rlap_bias_act_dropout, rlap_layer_norm
// and their _backward calls): the interface
// between rlap_rowops.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle,
// its lock and its arena.  The rule is in rlap_rowops.h.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct RowopsArgs {
    const float* x; int64_t L, N, F;          // (L, N, F)
    const float* gy;                          // backward: the upstream gradient (L, N, F)
    const float* weight;                      // layer norm: (F) or null: 1
    const float* bias;                        // (F) or null: 0
    const float* slope;                       // one value, or (F) with RLAP_ROW_SLOPE_PER_CHANNEL; null without PReLU
    double p; uint64_t seed;
    double eps;                               // layer norm
    int flags;                                // RLAP_ROW_* (include/rlap_hip.h)
    float* out;                               // forward: y; backward: gx (nullable); (L, N, F)
    float* gweight; float* gbias; float* gslope;   // backward: (F) (layer norm), (F), (1) or (F); null ones are skipped
};

struct RowopsReport { int vec; int64_t chunks; int launches; int instance; };

// arena bytes of a call
size_t rowops_bytes(const RowopsArgs& a, bool backward);
// the calls on `stream`; no host synchronisation; return an RLAP_* status
int rowops_run(hipStream_t stream, void* ws, size_t ws_bytes, const RowopsArgs& a, RowopsReport* rep);
int rowops_backward_run(hipStream_t stream, void* ws, size_t ws_bytes, const RowopsArgs& a, RowopsReport* rep);
// the same for the layer norm
size_t ln_bytes(const RowopsArgs& a, bool backward);
int ln_run(hipStream_t stream, void* ws, size_t ws_bytes, const RowopsArgs& a, RowopsReport* rep);
int ln_backward_run(hipStream_t stream, void* ws, size_t ws_bytes, const RowopsArgs& a, RowopsReport* rep);

}  // namespace rlap
