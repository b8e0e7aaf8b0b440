// rlap_readout.h -- the per-graph readout of batched node embeddings (rlap_graph_readout, rlap_readout.hip): what one
// element is, the arithmetic that maps the work of a call to (graph, chunk), and the rule that chooses the kernel.  Plain __host__ __device__ functions without any
// HIP dependency, as rlap_spmm.h: tests/csrc/readout_map_main.cc compiles this file with g++ under the sanitizers and checks the map
// exhaustively; the kernels read the same functions.
//
// y[l, g, f] is rlap_spmm.h's rule on the list of graph g's ids [node_ptr[g], node_ptr[g+1]) in increasing order, every coefficient
// 1.0, no loop term: float64 terms, chunks of spmm::CHUNK ids summed from 0 in list order, the chunk sums added to 0 in chunk order.
// The mean is that sum divided once, in float64, by the number of ids; an empty graph gives exactly 0 either way.  A float32
// result is the float64 value rounded once.
#pragma once
#include <stdint.h>

#include "rlap_spmm.h"

namespace rlap {
namespace readout {

RLAP_SPMM_HD int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the ids of graph g, [*s, *s + *n), inside [0, N) whatever the table holds (a well-formed table is returned as it is)
RLAP_SPMM_HD void graph_range(const int64_t* node_ptr, int64_t g, int64_t N, int64_t* s, int64_t* n) {
    *s = clampi(node_ptr[g], 0, N);
    *n = clampi(node_ptr[g + 1], *s, N) - *s;
}

// chunks of a graph of n ids; those of them that go through the arena (a graph of at most CHUNK ids finishes in one pass)
RLAP_SPMM_HD int32_t graph_chunks(int64_t n) { return (int32_t)spmm::num_chunks(n); }
RLAP_SPMM_HD int32_t graph_part_chunks(int64_t n) { return n > spmm::CHUNK ? (int32_t)spmm::num_chunks(n) : 0; }

// What the host knows of a well-formed table without reading it: G graphs over N ids have at most ceil(N / CHUNK) + G chunks
// (every graph ends at most one chunk that is not full), at most min(G, N / (CHUNK + 1)) of them are longer than one chunk, and
// those have at most ceil(N / CHUNK) + that many chunks.
RLAP_SPMM_HD int64_t chunk_bound(int64_t N, int64_t G) { return (N + spmm::CHUNK - 1) / spmm::CHUNK + G; }
RLAP_SPMM_HD int64_t chunked_bound(int64_t N, int64_t G) { const int64_t b = N / (spmm::CHUNK + 1); return b < G ? b : G; }
RLAP_SPMM_HD int64_t part_bound(int64_t N, int64_t G) {
    return N > spmm::CHUNK ? (N + spmm::CHUNK - 1) / spmm::CHUNK + chunked_bound(N, G) : 0;
}

// Work item q of a call: with choff[g] = the chunks of the graphs in front of g (choff[G] = all of them), the graph g that owns
// chunk q and q's number k within it.  The last g with choff[g] <= q: graphs without chunks are stepped over.  False outside
// [0, choff[G]).
RLAP_SPMM_HD bool item_of(const int64_t* choff, int64_t G, int64_t q, int64_t* g, int64_t* k) {
    if (q < 0 || G < 1 || q >= choff[G]) return false;
    int64_t lo = 0, hi = G;   // choff[lo] <= q < choff[hi]
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (choff[mid] <= q) lo = mid; else hi = mid;
    }
    *g = lo;
    *k = q - choff[lo];
    return true;
}

// Which kernel a call takes (launch_readout / launch_backward of rlap_readout.hip): a row of F elements of `elem_bytes` (4 or 8)
// takes 16 bytes a lane (`vec`) when F is a multiple of V = 16 / elem_bytes and both pointers lie on the 16-byte grid, else one
// element a lane.  `lg` is the smallest value with 2^lg >= lanes, capped at 6: below 6 the staged kernel for narrow rows runs with
// groups of 2^lg lanes, at 6 the kernel of one wave a row with `ftiles` tiles of 64 lanes.  The backward call reads vec and lanes.
struct Dispatch { bool vec; int64_t lanes; int lg; int64_t ftiles; };
RLAP_SPMM_HD Dispatch dispatch(int64_t F, int elem_bytes, bool aligned16) {
    const int64_t V = 16 / elem_bytes;
    Dispatch d;
    d.vec = aligned16 && F % V == 0;
    d.lanes = d.vec ? F / V : F;
    d.lg = 0;
    while (d.lg < 6 && ((int64_t)1 << d.lg) < d.lanes) ++d.lg;
    d.ftiles = (d.lanes + 63) >> 6;
    return d;
}

// the definition of one element: feat(e) is the feature of the e-th id of the graph
template <class Feat>
RLAP_SPMM_HD double graph_sum(int64_t n, Feat feat) {
    return spmm::list_sum(n, [](int64_t) { return 1.0; }, feat, false, 0.0, 0.0);
}

// the value stored for a graph of n ids whose sum is `total`
RLAP_SPMM_HD double finish(double total, int64_t n, bool mean) { return (mean && n > 0) ? total / (double)n : total; }

}  // namespace readout
}  // namespace rlap
