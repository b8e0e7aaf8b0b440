// rlap_edgeplan.h -- propagation plans for rows in any order (rlap_edge_plan_build).  Two parts:
//   1. the degree rule as plain __host__ __device__ functions without any HIP dependency: tests/csrc/edgeplan_mirror.cc compiles
//      them with g++ and builds a whole plan on the host; the kernels of rlap_edgeplan.hip read the same functions;
//   2. (HIP only) the interface between rlap_edgeplan.hip, which holds the kernels and their orchestration, and the C ABI in
//      rlap_api.hip, which owns the handle, its lock and its arena.
// The input is a row table [i, j, w] whose segments hold their rows in ANY order: duplicates, directed structure, loop rows and ids
// without rows are legal.  The lists of a plan are then defined by a row's place in the input alone:
//   forward list of (layer, j)    : the rows of the layer with target (column id) j, in input order;
//   transposed list of (layer, i) : the rows with source (row id) i, in input order;
//   loop rows that the flags drop are in neither.
// The degree of (layer, j) is k_gc_degree's rule (rlap_gcn.hip) restated over the target's list.  Let k be a row's place in the
// forward list, loop rows counted.  The row goes to lane k % 16, accumulator (k / 16) % 4, in ascending k (with self loops a loop
// row adds nothing); per lane (a0 + a1) + (a2 + a3); an xor butterfly over 8, 4, 2, 1 lanes; then the loop's weight (that of the
// list's last loop row, or fill) last.  dis = gcnmath::dis(deg).  An id without incoming rows has the loop's weight alone, or 0.
// For an input in the elimination layout a block's rows are its target's list, so the plan equals rlap_snapshot_plan_build's bit
// for bit.  Coefficients (rlap_gcnmath.h), list layout (rlap_plan.h) and summation order (rlap_spmm.h) are those headers'.
//
// Limits (reported as RLAP_E_TOO_LARGE, never truncated): m < 2^31 - 1 rows (positions and row numbers are int32) and
// (S / G) * num_nodes < 2^31 slots (the sort keys are uint32 and every slot has int32 range tables).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rlap_spmm.h"

namespace rlap {
namespace edgeplan {

constexpr int LANES = 16;      // lanes that share one list
constexpr int ACCS = 4;        // accumulators of a lane (loads in flight)
constexpr int64_t MAX_SLOTS = (int64_t)1 << 31;

// place k of a list <-> (turn of the lane, accumulator, lane)
RLAP_SPMM_HD int lane_of(int64_t k) { return (int)(k % LANES); }
RLAP_SPMM_HD int acc_of(int64_t k) { return (int)((k / LANES) % ACCS); }
RLAP_SPMM_HD int64_t place_of(int64_t turn, int acc, int lane) { return (turn * ACCS + acc) * LANES + lane; }

// the four accumulators of a lane
RLAP_SPMM_HD double combine(const double (&a)[ACCS]) { return (a[0] + a[1]) + (a[2] + a[3]); }

// one butterfly step: what a lane holds after it has met its partner (lane ^ o)
RLAP_SPMM_HD double meet(double mine, double partners) { return mine + partners; }

// the degree once the lanes are reduced: the loop's weight comes last
RLAP_SPMM_HD double finish(double sum, bool loops, double loop_w) { return loops ? sum + loop_w : sum; }

// bits of the sort keys: the slots are [0, slots)
RLAP_SPMM_HD unsigned key_bits(int64_t slots) {
    unsigned b = 1;
    while (b < 32 && ((int64_t)1 << b) < slots) ++b;
    return b;
}

// The whole rule over one list of n places, sequentially (the host's form; the kernel runs the same functions 16 lanes wide).
// weight(k) is the weight of place k, is_loop(k) whether it is a loop row; loops: RLAP_GCN_SELF_LOOPS.  *loop_w gets the loop's
// weight (fill unless the list has a loop row and loops is set).
template <class Weight, class IsLoop>
inline double degree(int64_t n, Weight weight, IsLoop is_loop, bool loops, double fill, double* loop_w) {
    double acc[LANES][ACCS];
    for (int l = 0; l < LANES; ++l)
        for (int u = 0; u < ACCS; ++u) acc[l][u] = 0.0;
    double w = fill;
    for (int64_t k = 0; k < n; ++k) {
        if (loops && is_loop(k)) { w = weight(k); continue; }
        acc[lane_of(k)][acc_of(k)] += weight(k);
    }
    double v[LANES];
    for (int l = 0; l < LANES; ++l) v[l] = combine(acc[l]);
    for (int o = LANES / 2; o > 0; o >>= 1) {
        double t[LANES];
        for (int l = 0; l < LANES; ++l) t[l] = meet(v[l], v[l ^ o]);
        for (int l = 0; l < LANES; ++l) v[l] = t[l];
    }
    *loop_w = w;
    return finish(v[0], loops, w);
}

}  // namespace edgeplan
}  // namespace rlap

#if defined(__HIPCC__) || defined(__HIP__)
#include "rlap_plan.h"

namespace rlap {

// arena bytes of the build (the plan buffer's bound is snapshot_plan_buffer_bytes: the layout is the same)
size_t edge_plan_build_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int flags);
// the build on `stream`, with `ws` as its scratch; fills *desc on success; returns an RLAP_* status.  rep->blocks is the number of
// non-empty forward lists.
int edge_plan_build_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotPlanArgs& a, rlap_plan_desc* desc,
                        SnapshotPlanReport* rep);

}  // namespace rlap
#endif
