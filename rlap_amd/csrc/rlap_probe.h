// rlap_probe.h -- the rule of the linear-probe evaluator (rlap_linear_probe / rlap_probe_scores, rlap_probe.hip): every
// value of the call and the order of every sum.  Plain __host__ __device__ functions without any HIP dependency, as rlap_cca.h and
// rlap_infonce.h: tests/csrc/probe_mirror.cc compiles this file with g++ (contraction off, as the library) and computes the same
// bits; tests/csrc/probe_main.cc runs the index arithmetic under the sanitizers; the kernels read the same functions.
//
// Inputs: x (N, F) float32, 1 <= F <= 512; labels y in [0, C), 2 <= C <= 64; R runs, each with a training, a validation and a test
// list of row indices (any order, repeats count twice, a sum over a list runs in list order); the initial W (C, F) and b (C) of
// every run; epochs, lr, weight_decay, beta1, beta2, eps.  A run is LREvaluator's loop (scripts/node_shared.py:163-230) or
// CCA-SSG/main.py:152-194's: full-batch Adam on a Linear(F, C) under log-softmax + NLL.  Per epoch t = 1 .. epochs, with i over
// the n training rows of the run in list order:
//
//   logits      z_ic = b_c + the float32 fmaf chain over k = 0 .. F-1 in increasing k from +0: acc = fmaf(x_ik, w_ck, acc) -- what
//               v_mfma_f32_32x32x2_f32 computes with k as the feature.  A padding column would be fmaf(0, 0, acc); the kernels stop at F.
//   softmax     m_i = max_c z_ic;  e_ic = expw(max(z_ic - m_i, EXP_MIN)) with rlap_infonce.h's expw (the argument is <= 0);
//               Z_i = the float64 sum over c = 0 .. C-1 in increasing order from 0 of (double)e_ic;  p_ic = (float)((double)e_ic / Z_i);
//               g_ic = p_ic - [c = y_i] in float32.  The loss term of the row is log(Z_i) - ((double)z_i,y_i - (double)m_i) in
//               float64: the only library transcendental of the call, and it feeds nothing but the reported loss.
//   gradients   dW_ck = 0 + part 0 + part 1 + ... in float64, a part being the float32 fmaf chain over its training rows in list
//               order from +0: acc = fmaf(g_ic, x_ik, acc).  The parts are runs of whole 256-row chunks of the list, a function of
//               (n, F, C) alone (num_parts, part_begin); the rows behind n that fill the last 32-row tile take no turn.
//               db_c = rlap_spmm.h's chunk rule over the rows of 1 * (double)g_ic.  Both are divided by n in float64 and rounded to
//               float32 once.  loss = (chunk rule over the rows of 1 * term_i) / n, float64.
//   Adam        torch's formula, L2 weight decay added to the gradient, operation by operation in float32 (adam_step below); the
//               bias corrections 1 - beta^t come from float64 running products (AdamCoef::advance), never from pow.  A float32
//               quotient or root is formed in float64 and rounded once, which is the correctly rounded float32 result.
//               The claim is closeness to a float64 restatement, not the bits of any torch implementation.
//   scoring     z as above for the listed rows; the prediction is the lowest index among the largest logits (argmax's rule);
//               confusion[true][predicted] counts rows with integer atomics, which commute.  accuracy = micro_f1 = trace / rows;
//               macro_f1 = the plain mean, in increasing label order, of 2 tp / (2 tp + fp + fn) over the labels that occur among
//               the true or the predicted labels (sklearn's default label set).  float64 functions of integers.
//   selection   SELECT_SCRIPTS: after the step of every epoch e (from 0) with (e + 1) % test_interval == 0: when val_correct >
//               best_val (initially 0), best_val = val_correct and the test scores, the confusion matrices and e are recorded.
//               SELECT_CCA: after every step: when val_correct >= best_val: best_val = val_correct, and when test_correct >
//               best_test (initially 0): best_test = test_correct and the same things are recorded.  The rules compare integer
//               counts of correct rows; the denominators are fixed, so below 2^24 rows this equals the reference's comparison of
//               float32 ratios.  Nothing recorded leaves scores of 0, epoch 0 and zero matrices, as the reference's initial values.
#pragma once
#include <math.h>
#include <stdint.h>

#include "rlap_infonce.h"
#include "rlap_spmm.h"
#include "rlap_tile32.h"

namespace rlap {
namespace probe {

using tile32::TILE;                       // training rows a workgroup holds at a time: rlap_tile32.h's tile
using tile32::num_tiles;
using tile32::padded_rows;
constexpr int MAX_F = 512;                // feature columns of a call
constexpr int MAX_C = 64;                 // classes of a call
constexpr int MIN_CP = 8;                 // the class count is padded to 8, 16, 32 or 64 in the kernels' images
constexpr int MAX_RUNS = 32;              // runs of a call (their tables travel as kernel arguments)
constexpr int64_t MAX_PARTS = 64;         // parts of a run's training list (bounds the partial sums of the arena)
constexpr float EXP_MIN = -80.0f;         // the clamp of expw's argument: expw(-80) is a normal float32
enum { SELECT_SCRIPTS = 0, SELECT_CCA = 1 };
// what the kernels raise in the call's status word on the device (the values of RLAP_E_INDEX_RANGE and RLAP_E_BAD_ARG): an index
// outside [0, N) -- row 0 is read in its place --, a label outside [0, C) -- the row then marks no class and is not counted
enum { STATUS_OK = 0, STATUS_INDEX = 2, STATUS_LABEL = 3 };
// rlap_probe_info.detail: which host-side check refused the call
enum { DETAIL_OK = 0, DETAIL_SHAPE = 1, DETAIL_LIST = 2, DETAIL_PARAM = 3, DETAIL_POINTER = 4 };

RLAP_SPMM_HD bool finite_ok(double v) { return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308; }   // (false for a NaN)

RLAP_SPMM_HD int class_pad(int64_t C) { int p = MIN_CP; while (p < C && p < MAX_C) p *= 2; return p; }
// the row stride of a training image and of the step's tile in LDS, in floats: odd, so that rows fall into different banks
RLAP_SPMM_HD int64_t image_stride(int64_t F) { return F | 1; }

// The parts of a training list of n rows: runs of whole chunks, as many as there are chunks, at most MAX_PARTS.  A function of
// (n, F, C) alone (today of n alone).
RLAP_SPMM_HD int64_t num_parts(int64_t n, int64_t F, int64_t C) {
    (void)F; (void)C;
    const int64_t nc = spmm::num_chunks(n);
    return nc < 1 ? 1 : (nc > MAX_PARTS ? MAX_PARTS : nc);
}
// first chunk of part p (p <= num_parts); the part's rows are [part_begin, part_end), the last part ending at n
RLAP_SPMM_HD int64_t part_chunk(int64_t n, int64_t F, int64_t C, int64_t p) { return p * spmm::num_chunks(n) / num_parts(n, F, C); }
RLAP_SPMM_HD int64_t part_begin(int64_t n, int64_t F, int64_t C, int64_t p) {
    const int64_t r = part_chunk(n, F, C, p) * spmm::CHUNK;
    return r < n ? r : n;
}
RLAP_SPMM_HD int64_t part_end(int64_t n, int64_t F, int64_t C, int64_t p) { return part_begin(n, F, C, p + 1); }

// ---- the values
RLAP_SPMM_HD float chain_step(float acc, float a, float b) { return fmaf(a, b, acc); }
RLAP_SPMM_HD float logit_of(float bias, float chain) { return bias + chain; }
// the logits of one row: w is (C, F) row-major
RLAP_SPMM_HD void row_logits(const float* x, const float* w, const float* b, int64_t F, int64_t C, float* z) {
    for (int64_t c = 0; c < C; ++c) {
        float acc = 0.0f;
        for (int64_t k = 0; k < F; ++k) acc = chain_step(acc, x[k], w[c * F + k]);
        z[c] = logit_of(b[c], acc);
    }
}
RLAP_SPMM_HD float exp_term(float z, float m) {
    float a = z - m;
    if (a < EXP_MIN) a = EXP_MIN;
    return infonce::expw(a);
}
RLAP_SPMM_HD float prob_of(float e, double Z) { return (float)((double)e / Z); }
RLAP_SPMM_HD float grad_logit(float p, bool is_label) { return p - (is_label ? 1.0f : 0.0f); }
RLAP_SPMM_HD double loss_term(double Z, float zy, float m) { return log(Z) - ((double)zy - (double)m); }
// the softmax of one row in place: z (C logits) becomes g; returns the loss term.  A label outside [0, C) marks no class (the call
// reports it) and takes 0 as its logit.
RLAP_SPMM_HD double row_softmax(float* z, int64_t C, int64_t label) {
    float m = z[0];
    for (int64_t c = 1; c < C; ++c) m = z[c] > m ? z[c] : m;
    const float zy = (label >= 0 && label < C) ? z[label] : 0.0f;
    double Z = 0.0;
    for (int64_t c = 0; c < C; ++c) { z[c] = exp_term(z[c], m); Z = Z + (double)z[c]; }
    for (int64_t c = 0; c < C; ++c) z[c] = grad_logit(prob_of(z[c], Z), c == label);
    return loss_term(Z, zy, m);
}
RLAP_SPMM_HD int predict(const float* z, int64_t C) {
    int best = 0;
    for (int64_t c = 1; c < C; ++c) if (z[c] > z[best]) best = (int)c;
    return best;
}
RLAP_SPMM_HD float mean_grad(double total, int64_t n) { return (float)(total / (double)n); }

// a float32 quotient and root through float64: correctly rounded, whatever the compiler makes of a float32 division
RLAP_SPMM_HD float fdiv(float a, float b) { return (float)((double)a / (double)b); }
RLAP_SPMM_HD float fsqrt(float a) { return (float)sqrt((double)a); }

struct AdamCoef {
    double beta1, beta2, lr, b1p, b2p;      // b1p, b2p: beta^t, running products
    float b1, omb1, b2, omb2, eps, wd;      // the float32 constants of a step
    float step, rbc2;                       // lr / (1 - beta1^t) and sqrt(1 - beta2^t) of the current epoch
    RLAP_SPMM_HD void init(double lr_, double wd_, double beta1_, double beta2_, double eps_) {
        beta1 = beta1_; beta2 = beta2_; lr = lr_; b1p = 1.0; b2p = 1.0;
        b1 = (float)beta1_; omb1 = (float)(1.0 - beta1_); b2 = (float)beta2_; omb2 = (float)(1.0 - beta2_);
        eps = (float)eps_; wd = (float)wd_; step = 0.0f; rbc2 = 1.0f;
    }
    RLAP_SPMM_HD void advance() {           // to the next epoch t
        b1p = b1p * beta1; b2p = b2p * beta2;
        step = (float)(lr / (1.0 - b1p));
        rbc2 = (float)sqrt(1.0 - b2p);
    }
};
// one parameter's step: g the mean gradient; w, m, v in place
RLAP_SPMM_HD void adam_step(const AdamCoef& a, float g, float* w, float* m, float* v) {
    if (a.wd != 0.0f) { const float t = a.wd * *w; g = g + t; }
    const float m1 = a.b1 * *m, m2 = a.omb1 * g;
    *m = m1 + m2;
    const float gg = g * g;
    const float v1 = a.b2 * *v, v2 = a.omb2 * gg;
    *v = v1 + v2;
    const float denom = fdiv(fsqrt(*v), a.rbc2) + a.eps;
    const float u = a.step * fdiv(*m, denom);
    *w = *w - u;
}

// ---- the scores of a (C, C) confusion matrix, rows true, columns predicted
template <class Int>
RLAP_SPMM_HD int64_t correct_of(const Int* conf, int64_t C) {
    int64_t t = 0;
    for (int64_t c = 0; c < C; ++c) t += (int64_t)conf[c * C + c];
    return t;
}
RLAP_SPMM_HD double f1_of(int64_t tp, int64_t row_sum, int64_t col_sum) {   // 2 tp / (2 tp + fp + fn); row_sum + col_sum > 0
    return (double)(2 * tp) / (double)(row_sum + col_sum);
}
template <class Int>
RLAP_SPMM_HD void scores_of(const Int* conf, int64_t C, int64_t rows, double* micro, double* macro, double* accuracy) {
    double total = 0.0;
    int64_t present = 0;
    for (int64_t c = 0; c < C; ++c) {
        int64_t rs = 0, cs = 0;
        for (int64_t d = 0; d < C; ++d) { rs += (int64_t)conf[c * C + d]; cs += (int64_t)conf[d * C + c]; }
        if (rs + cs > 0) { total = total + f1_of((int64_t)conf[c * C + c], rs, cs); ++present; }
    }
    const double acc = rows > 0 ? (double)correct_of(conf, C) / (double)rows : 0.0;
    *micro = acc; *accuracy = acc;
    *macro = present > 0 ? total / (double)present : 0.0;
}

// ---- the selection rule
struct Record { int64_t best_val, best_test, epoch, recorded; };
RLAP_SPMM_HD bool scoring_epoch(int select, int64_t epoch, int64_t test_interval) {
    return select == SELECT_CCA || (epoch + 1) % test_interval == 0;
}
// whether the evaluation of `epoch` is recorded; updates the record
RLAP_SPMM_HD bool select_take(int select, int64_t val_correct, int64_t test_correct, int64_t epoch, Record* r) {
    bool take = false;
    if (select == SELECT_CCA) {
        if (val_correct >= r->best_val) {
            r->best_val = val_correct;
            if (test_correct > r->best_test) { r->best_test = test_correct; take = true; }
        }
    } else if (val_correct > r->best_val) {
        r->best_val = val_correct; r->best_test = test_correct; take = true;
    }
    if (take) { r->epoch = epoch; r->recorded = 1; }
    return take;
}

}  // namespace probe
}  // namespace rlap
