// rlap_probe_api.h -- the linear-probe evaluator (rlap_linear_probe / rlap_probe_scores): the interface between
// rlap_probe.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock and
// its arena.  The rule is rlap_probe.h's.
#pragma once
#include "rlap_snapshot.h"

namespace rlap {

struct ProbeArgs {
    const float* x; int64_t N, F, ldx;              // (N, F) float32 on the device, rows ldx floats apart
    const int64_t* y; int64_t C, R;                 // [N] labels on the device; classes; runs
    const int64_t* idx[3]; const int64_t* hptr[3];  // training, validation, test: the runs' lists on the device, their [R+1] offsets on the HOST
    int64_t epochs, test_interval; int select;      // (scores_run reads idx[0] / hptr[0] alone)
    double lr, wd, beta1, beta2, eps;
    const float* w0; const float* b0;               // (R, C, F), (R, C): the initial parameters (scores_run: the parameters)
    // results
    float* w; float* b;                             // the final parameters
    double* scores;                                 // (R, 4): micro_f1, macro_f1, accuracy, loss (scores_run: (R, 3))
    int64_t* best;                                  // (R, 2): the recorded epoch, its validation count
    int64_t* confusion;                             // (R, 2, C, C): validation, test (scores_run: (R, C, C))
    int64_t* pred;                                  // scores_run: one prediction per listed row
    int32_t* status;                                // one word: 0, or what the kernels found (probe::STATUS_*)
};

// the host-side checks of the lists' offsets: first 0, strictly increasing (no empty list); the largest number of parts and tiles
bool probe_lists_ok(const int64_t* hptr, int64_t R);
// arena bytes of the two calls (the offsets checked)
size_t probe_bytes(const ProbeArgs& a);
size_t scores_bytes(const ProbeArgs& a);
// the calls on `stream`; no host synchronisation; return an RLAP_* status; *launches counts the kernels enqueued
int probe_run(hipStream_t stream, void* ws, size_t ws_bytes, const ProbeArgs& a, int64_t* parts, int64_t* launches);
int scores_run(hipStream_t stream, void* ws, size_t ws_bytes, const ProbeArgs& a, int64_t* launches);

}  // namespace rlap
