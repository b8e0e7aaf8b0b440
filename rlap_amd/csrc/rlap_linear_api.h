// rlap_linear_api.h -- the fused dense layer (rlap_linear_act / rlap_linear_act_backward): the interface between
// rlap_linear.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock
// and its arena.  The rule is rlap_linear.h's.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct LinearArgs {
    const float* x; const float* w; const float* b;   // x (M, Fin); w (Fin, Fout), or (Fout, Fin) with WEIGHT_OUT_IN; b (Fout,) or null
    int64_t M, Fin, Fout;
    int act; double alpha; int flags;
    float* y;                                         // forward: the result (M, Fout)
    // backward: the forward's result and the upstream gradient, (M, Fout) each; results, each nullable: gx (M, Fin), gw of w's
    // layout, gb (Fout,)
    const float* y_in; const float* gy; float* gx; float* gw; float* gb;
};

// arena bytes of the two calls (the backward's for the gradients that are asked for)
size_t linear_bytes(int64_t M, int64_t Fin, int64_t Fout);
size_t linear_backward_bytes(int64_t M, int64_t Fin, int64_t Fout, bool gx, bool gw, bool gb);
// the calls on `stream`; no host synchronisation; return an RLAP_* status
int linear_run(hipStream_t stream, void* ws, size_t ws_bytes, const LinearArgs& a);
int linear_backward_run(hipStream_t stream, void* ws, size_t ws_bytes, const LinearArgs& a);

}  // namespace rlap
