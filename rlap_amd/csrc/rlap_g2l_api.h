// rlap_g2l_api.h -- the fused graph-to-local losses (rlap_g2l_jsd / rlap_g2l_bootstrap and their backward calls): the
// interface between rlap_g2l.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the
// handle, its lock and its arena.  The rule is rlap_g2l.h's.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct G2lArgs {
    const float* h; const float* neg; const float* g;   // (N, F), (N, F) or nullptr, (G, F) float32 on the device
    int64_t N, F; const int64_t* node_ptr; int64_t G;   // [G+1] on the device, never read back
    // forward: results
    double* loss; double* rows;                         // one double; JSD [2 N]: pos_i, neg_i; bootstrap [N]: c_i
    // backward: the upstream scalar on the device; results (N, F), (N, F) or nullptr, (G, F)
    const double* gup; float* gh; float* gneg; float* gg;
};

// arena bytes of a call (g2l::Call)
size_t g2l_bytes(int call, int64_t N, int64_t G, int64_t F);
// the calls on `stream`; no host synchronisation; return an RLAP_* status
int g2l_run(int call, hipStream_t stream, void* ws, size_t ws_bytes, const G2lArgs& a);

}  // namespace rlap
