// rlap_edgeadd.h -- edge adding, K views a call (rlap_edge_add).  Two parts:
//   1. the rules as plain __host__ __device__ functions without any HIP dependency: tests/csrc/edgeadd_mirror.cc compiles them
//      with g++ and runs a whole call on the host; the kernels of rlap_edgeadd.hip read the same functions;
//   2. (HIP only) the interface between rlap_edgeadd.hip, which holds the kernels and their orchestration, and the C ABI in
//      rlap_api.hip, which owns the handle, its lock and its arena.
// The input is E rows (source, target) in any order; duplicates, loops and directed rows are allowed.  View k adds num_add[k] rows
// drawn uniformly from [0, N - 2]^2 (scripts/augmentor_benchmarks.py:44-54: torch.randint's upper end N - 1 is exclusive, so the
// last node never receives an added row; restated as it stands) and, with coalesce, sorts and merges the lot.  Everything is
// integer arithmetic, one float64 multiply a draw and float64 additions in a stated order, so the device and the host mirror agree
// in every bit.
//   coin     u_add(k, i, c) = coin_of(mix64((seed + k) ^ ADD_SALT), mix64(2 i + c)), added row i of view k, c = 0 source, 1 target
//   draw     added row i of view k = (pick(u_add(k, i, 0), N - 1), pick(u_add(k, i, 1), N - 1)), nodesample::pick
//   key      key(s, t) = (s << b) | t with b = id_bits(N), the least b >= 1 with 2^b >= N; keys ascend as (source, target) does
//   merge    the distinct keys of the input (list A) and those of a view's added rows (list B) are merged ascending; of two equal
//            keys A's comes first (takes_a)
//   weight   of a pair: s_in + (double)c_add in one addition (weight); s_in = the sum of the pair's input rows, from 0.0 in input
//            order (run_add; 1.0 a row without weights; 0.0 without rows), c_add = the pair's added rows
//   without coalesce a view is the E input rows in input order, then its added rows in draw order with weight 1.0.
//
// Limits (RLAP_E_TOO_LARGE, never truncated): E + max num_add < 2^31 - 1, num_nodes < 2^31, K <= 32.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rlap_core.h"
#include "rlap_edgedrop.h"
#include "rlap_nodesample.h"

namespace rlap {
namespace edgeadd {

constexpr int TILE = edgedrop::TILE;             // threads of a workgroup
constexpr int WAVE = edgedrop::WAVE;
constexpr int ROW_TILE = edgedrop::ROW_TILE;     // merged positions a workgroup owns
constexpr int PER_LANE = ROW_TILE / TILE;        // consecutive merged positions of a lane
constexpr int MAX_VIEWS = edgedrop::MAX_VIEWS;
constexpr uint64_t ADD_SALT = 0x6564676561646473ull;   // not COIN_SALT, NODE_SALT or WALK_SALT: an added view of a seed shares no coin with them

// ---- the coin and the draw
RLAP_SPMM_HD uint64_t add_view(uint64_t seed, int k) { return mix64((seed + (uint64_t)k) ^ ADD_SALT); }
RLAP_SPMM_HD double u_add(uint64_t view, int64_t i, int c) { return edgedrop::coin_of(view, mix64(2 * (uint64_t)i + (uint64_t)c)); }
// end c of added row i: an id in [0, N - 2] (N >= 2)
RLAP_SPMM_HD int64_t draw(uint64_t view, int64_t i, int c, int64_t N) { return nodesample::pick(u_add(view, i, c), N - 1); }

// ---- the key of a pair
RLAP_SPMM_HD unsigned id_bits(int64_t N) {
    unsigned b = 1;
    while (b < 31 && ((int64_t)1 << b) < N) ++b;
    return b;
}
RLAP_SPMM_HD unsigned key_width(int64_t N) { return 2 * id_bits(N); }
RLAP_SPMM_HD uint64_t pair_key(int64_t s, int64_t t, unsigned b) { return ((uint64_t)s << b) | (uint64_t)t; }
RLAP_SPMM_HD int64_t key_source(uint64_t key, unsigned b) { return (int64_t)(key >> b); }
RLAP_SPMM_HD int64_t key_target(uint64_t key, unsigned b) { return (int64_t)(key & (((uint64_t)1 << b) - 1)); }
// bits of the view number beside a key, and whether one sort serves all K views' added rows
RLAP_SPMM_HD unsigned view_bits(int K) {
    unsigned v = 0;
    while (((int)1 << v) < K) ++v;
    return v;
}
// (bit 63 stays clear: no key, with or without a view number, is the all-ones word)
RLAP_SPMM_HD bool one_sort(int64_t N, int K) { return key_width(N) + view_bits(K) <= 63; }

// ---- the merge and the weight
RLAP_SPMM_HD bool takes_a(uint64_t a, uint64_t b) { return a <= b; }   // of two equal keys the input's comes first
RLAP_SPMM_HD double run_add(double s, double w) { return s + w; }      // s_in: from 0.0, a row at a time in input order
RLAP_SPMM_HD double weight(double s_in, int64_t c_add) { return s_in + (double)c_add; }

// how many of the first d merged entries are A's: A is [0, na), B is [0, nb), both ascending, 0 <= d <= na + nb
template <class KeyA, class KeyB>
RLAP_SPMM_HD int64_t merge_split(int64_t d, int64_t na, int64_t nb, KeyA a, KeyB b) {
    int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (takes_a(a(mid), b(d - 1 - mid))) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace edgeadd
}  // namespace rlap

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

namespace rlap {

struct EdgeAddArgs {
    const int64_t* src; const int64_t* dst; const double* w; int64_t E, N;
    int K, coalesce;
    int64_t num_add[edgeadd::MAX_VIEWS]; uint64_t seed;
    double* rows; int64_t cap; int64_t* ptr;   // (cap, 3) and [K + 1]
    int64_t* added; int64_t* aptr;             // optional, both or neither: (sum of num_add, 2) and [K + 1]
};
struct EdgeAddReport { int64_t rows_needed, added, input_distinct, launches; int32_t input_sorted, sorts, host_syncs; };

size_t edge_add_bytes(int64_t E, int64_t N, int K, const int64_t* num_add, bool coalesce);
int edge_add_run(hipStream_t stream, void* ws, size_t ws_bytes, const EdgeAddArgs& a, EdgeAddReport* rep);

}  // namespace rlap
#endif
