// rlap_nodesample.h -- node dropping and random-walk subgraph views (rlap_node_sample).  Two parts:
//   1. the rules as plain __host__ __device__ functions without any HIP dependency: tests/csrc/nodesample_mirror.cc compiles them
//      with g++ and runs a whole call on the host; the kernels of rlap_nodesample.hip read the same functions;
//   2. (HIP only) the interface between rlap_nodesample.hip, which holds the kernels and their orchestration, and the C ABI in
//      rlap_api.hip, which owns the handle, its lock and its arena.
// The input is E rows (source, target) in any order; duplicates, loops and directed structure stay as they are.  A view is a node
// set; row e is in view k iff its source and its target are both in the set (PyG's subgraph(subset, edge_index, edge_attr) with
// relabel_nodes=False: the ids stay).  Everything is integer arithmetic plus one float64 multiply, so the device and the host
// mirror agree in every bit.
//   node coin  u_node(k, v) = coin_of(mix64((seed + k) ^ NODE_SALT), mix64(v))
//   drop       node v is in the set of view k iff u_node(k, v) >= p[k]: PyGCL's NodeDropping(pn) keeps a node with probability
//              1 - pn; p = 0 keeps every node, p = 1 none
//   walk coin  u_walk(k, i, t) = coin_of(mix64((seed + k) ^ WALK_SALT), mix64(i * (walk_length + 1) + t)), walker i, step t
//   pick       pick(u, n) = min((int64)(u * (double)n), n - 1)
//   walk       v_0 = pick(u_walk(k, i, 0), N); for t = 1 .. walk_length: d = the rows whose source is v_{t-1} (duplicates and loops
//              counted); d == 0: v_t = v_{t-1} (the walker stays: torch_cluster's rule); otherwise v_t = the target of the
//              pick(u_walk(k, i, t), d)-th such row in input order of the rows.  The set of view k: every v_t of every walker.
// PyGCL, torch_sparse and torch_cluster are not run here: these are their published semantics restated.  The walk is uniform over
// a node's outgoing rows, the distribution of SparseTensor.random_walk, not its random stream.
//
// Limits (RLAP_E_TOO_LARGE, never truncated): E < 2^31 - 1, num_nodes < 2^31, K <= 32, num_seeds[k] < 2^31.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rlap_bitrank.h"
#include "rlap_core.h"
#include "rlap_edgedrop.h"

namespace rlap {
namespace nodesample {

constexpr int TILE = edgedrop::TILE;             // threads of a workgroup
constexpr int WAVE = edgedrop::WAVE;
constexpr int ROW_TILE = edgedrop::ROW_TILE;     // rows a workgroup flips and compacts
constexpr int MAX_VIEWS = edgedrop::MAX_VIEWS;
constexpr int64_t MAX_WALK_LENGTH = 1024;
constexpr uint64_t NODE_SALT = 0x6E6F646564726F70ull;   // not edgedrop::COIN_SALT: a node view and an edge view of one seed differ
constexpr uint64_t WALK_SALT = 0x72776C6B73616D70ull;
enum { DROP = 0, WALK = 1, SCHEMES = 2 };

// ---- the node coin and the drop decision
RLAP_SPMM_HD uint64_t node_view(uint64_t seed, int k) { return mix64((seed + (uint64_t)k) ^ NODE_SALT); }
RLAP_SPMM_HD uint64_t node_hash(int64_t v) { return mix64((uint64_t)v); }
RLAP_SPMM_HD double u_node(uint64_t view, int64_t v) { return edgedrop::coin_of(view, node_hash(v)); }
RLAP_SPMM_HD bool node_kept(uint64_t view, uint64_t hash, double p) { return edgedrop::coin_of(view, hash) >= p; }

// ---- the walk coin, the pick and a step
RLAP_SPMM_HD uint64_t walk_view(uint64_t seed, int k) { return mix64((seed + (uint64_t)k) ^ WALK_SALT); }
RLAP_SPMM_HD double u_walk(uint64_t view, int64_t i, int64_t t, int64_t walk_length) {
    return edgedrop::coin_of(view, mix64((uint64_t)i * (uint64_t)(walk_length + 1) + (uint64_t)t));
}
RLAP_SPMM_HD int64_t pick(double u, int64_t n) {
    const int64_t j = (int64_t)(u * (double)n);
    return j < n - 1 ? j : n - 1;
}
RLAP_SPMM_HD int64_t walk_start(uint64_t view, int64_t i, int64_t walk_length, int64_t N) { return pick(u_walk(view, i, 0, walk_length), N); }
// the place, inside the list of a node with d > 0 outgoing rows, of the row that step t of walker i follows
RLAP_SPMM_HD int64_t walk_place(uint64_t view, int64_t i, int64_t t, int64_t walk_length, int64_t d) { return pick(u_walk(view, i, t, walk_length), d); }

// ---- the node set of a view: bit v of K * words_for(N) words, view-major (rlap_bitrank.h's layout)
RLAP_SPMM_HD int64_t set_words(int64_t N) { return bitrank::words_for(N); }
RLAP_SPMM_HD bool set_test(const uint64_t* words, int64_t v) { return (words[v >> 6] >> (v & 63)) & 1; }

}  // namespace nodesample
}  // namespace rlap

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>

namespace rlap {

struct NodeSampleArgs {
    const int64_t* src; const int64_t* dst; const double* w; int64_t E, N;
    int scheme, K;
    double p[nodesample::MAX_VIEWS]; int64_t seeds[nodesample::MAX_VIEWS];   // drop: p[k]; walk: the walkers of view k
    int64_t walk_length; uint64_t seed;
    double* rows; int64_t cap; int64_t* ptr;   // (cap, 3) and [K + 1]
    uint8_t* node_mask; int64_t* walks;        // optional: (K, N) bytes, (sum of seeds, walk_length + 1)
};
struct NodeSampleReport { int64_t rows_needed, launches; int32_t host_syncs; };

size_t node_sample_bytes(int64_t E, int64_t N, int K, int scheme, bool node_mask);
int node_sample_run(hipStream_t stream, void* ws, size_t ws_bytes, const NodeSampleArgs& a, NodeSampleReport* rep);

}  // namespace rlap
#endif
