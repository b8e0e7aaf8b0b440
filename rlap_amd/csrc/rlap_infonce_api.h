// rlap_infonce_api.h -- the fused InfoNCE loss (rlap_infonce / rlap_infonce_backward): the interface between
// rlap_infonce.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock
// and its arena.  The rule is rlap_infonce.h's.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct InfonceArgs {
    const float* a; const float* b; int64_t N, F;   // anchor and sample, (N, F) float32 on the device
    double tau; int flags;                          // RLAP_INFONCE_POSITIVE_RAW (include/rlap_hip.h)
    // forward: results
    double* loss; double* rows; double* z;          // one double; N; N
    // backward: the forward's row sums, the upstream scalar on the device; results (N, F) each
    const double* z_in; const double* g; float* ga; float* gb;
    // intraview negatives: infonce::INTRA_NONE (the calls above), INTRA_MASKED or INTRA_ALL
    int intraview;
};

// arena bytes of the two calls
size_t infonce_bytes(int64_t N, int64_t F, int intraview = 0);
size_t infonce_backward_bytes(int64_t N, int64_t F, int intraview = 0);
// the calls on `stream`; no host synchronisation; return an RLAP_* status.  a.intraview selects the intraview variant of either call
// (rlap_infonce_intra and its kin); the arena queries take it too
int infonce_run(hipStream_t stream, void* ws, size_t ws_bytes, const InfonceArgs& a);
int infonce_backward_run(hipStream_t stream, void* ws, size_t ws_bytes, const InfonceArgs& a);

// the symmetric pair (rlap_infonce_pair / rlap_infonce_pair_backward): the same arguments, with rows, z and z_in
// [2, N] -- the anchors' list, then the samples'
size_t infonce_pair_bytes(int64_t N, int64_t F, int intraview = 0);
size_t infonce_pair_backward_bytes(int64_t N, int64_t F, int intraview = 0);
size_t infonce_pair_lds_bytes(int64_t N, int64_t F);   // dynamic LDS of the forward main kernel
int infonce_pair_run(hipStream_t stream, void* ws, size_t ws_bytes, const InfonceArgs& a);
int infonce_pair_backward_run(hipStream_t stream, void* ws, size_t ws_bytes, const InfonceArgs& a);

}  // namespace rlap
