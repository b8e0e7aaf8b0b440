// rlap_cca_api.h -- the fused CCA-SSG loss (rlap_cca_loss / rlap_cca_loss_backward): the interface between
// rlap_cca.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and
// its arena.  The rule is rlap_cca.h's.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct CcaArgs {
    const float* a; const float* b; int64_t N, F;   // the two views' embeddings, (N, F) float32 on the device
    double lambd;
    // forward: results
    double* terms; double* colstat; float* gram;    // 4 doubles: loss, inv, dec1, dec2; 4 F doubles: mean1, sd1, mean2, sd2; 2 F F floats: r1, r2
    // backward: the forward's column statistics and residuals, the upstream scalar on the device; results (N, F) each
    const double* colstat_in; const float* gram_in; const double* g; float* ga; float* gb;
};

// arena bytes of the two calls
size_t cca_bytes(int64_t N, int64_t F);
size_t cca_backward_bytes(int64_t N, int64_t F);
// the calls on `stream`; no host synchronisation; return an RLAP_* status
int cca_run(hipStream_t stream, void* ws, size_t ws_bytes, const CcaArgs& a);
int cca_backward_run(hipStream_t stream, void* ws, size_t ws_bytes, const CcaArgs& a);

}  // namespace rlap
