// rlap_nodesample.hip -- node dropping and random-walk subgraph views, K views a call (rlap_node_sample).  The rules --
// both coins, the pick, a walk's step and the node set's layout -- are rlap_nodesample.h's.  A translation unit of its own.
//
//   keys     one pass over the rows: both ids checked (a row that fails raises the error word; every later kernel returns on a raised
//            word); walk only: the source key and the row number for the sort.
//   lists    walk only: rocPRIM's stable radix sort of (source, row) gives every node's outgoing rows in input order; [lo, hi) per
//            node (hi - lo is out[v]), the 4-byte target ids stored in list order.
//   walk     one lane per (view, walker), walk_length dependent gathers, every index clamped into its array before use; the visited
//            nodes marked in the view's bitmap with integer atomicOr (a set of bits does not depend on the order of the marks); the
//            optional walks written with plain stores.
//   nodes    only for the optional node mask: drop builds the bitmap from the node coins, a word a wave (ballot, no atomic); the
//            bytes are then written from the bitmap for both schemes.
//   flip     the per-row kernels, rlap_rowcompact_dev.h's two passes (k_rc_count, k_rc_ptr, k_rc_write), all K views from one read
//            of the row's two ids.  The predicate of drop (NodeCoins): two node coins recomputed in registers; of walk (InWalk): two
//            bit tests in the view's bitmap.  Neither has a per-row mask.
//   One read-back: the error word and the row total.  No atomic on a float; LDS holds wave counts only.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_nodesample.h"
#include "rlap_rowcompact_dev.h"
#include "rlap_snapshot.h"

namespace rlap {
namespace {

using namespace nodesample;
using rowcompact::clamp;

constexpr int64_t NS_MAX_GRID = 8192;                    // workgroups of a strided launch
enum { W_ERR = 0, W_TOTAL64 = 1, W_WORDS64 = 2 };        // int32 word 0; the total is int64 word 1

inline unsigned ns_blocks(int64_t n) { return capped_blocks(n, TILE, NS_MAX_GRID); }

struct Ns {
    const int64_t* src; const int64_t* dst; int64_t E, N, W;   // W: words of one view's bitmap
    int K;
    int32_t* words;
    uint32_t* key; int32_t* val; int32_t* lo; int32_t* hi; int32_t* tgts;
    uint64_t* bits;                                            // [K * W]
    double p[MAX_VIEWS]; int64_t first[MAX_VIEWS + 1];         // walk: view k owns walkers [first[k], first[k + 1])
    int64_t walk_length; uint64_t seed;
    uint8_t* node_mask; int64_t* walks;
};

__device__ inline bool ns_failed(const Ns& a) { return a.words[W_ERR] != 0; }

__global__ __launch_bounds__(TILE) void k_ns_keys(Ns a, int csr) {
    for (int64_t e = (int64_t)blockIdx.x * TILE + threadIdx.x; e < a.E; e += (int64_t)gridDim.x * TILE) {
        const int64_t s = a.src[e], d = a.dst[e];
        const bool ok = s >= 0 && s < a.N && d >= 0 && d < a.N;
        if (!ok) atomicOr(&a.words[W_ERR], 1);
        if (csr) { a.key[e] = ok ? (uint32_t)s : 0u; a.val[e] = (int32_t)e; }
    }
}

// marks node v (0 <= v < N) in the bitmap of view k: an integer atomic only where the bit is not seen set
__device__ inline void ns_mark(const Ns& a, int k, int64_t v) {
    uint64_t* word = a.bits + (int64_t)k * a.W + (v >> 6);
    const uint64_t bit = (uint64_t)1 << (v & 63);
    if (!(__atomic_load_n(word, __ATOMIC_RELAXED) & bit)) atomicOr(reinterpret_cast<unsigned long long*>(word), (unsigned long long)bit);
}

// one lane per (view, walker)
__global__ __launch_bounds__(TILE) void k_ns_walk(Ns a) {
    if (ns_failed(a) || a.N < 1) return;
    const int64_t total = a.first[a.K], L = a.walk_length;
    for (int64_t g = (int64_t)blockIdx.x * TILE + threadIdx.x; g < total; g += (int64_t)gridDim.x * TILE) {
        int k = 0;
        while (k + 1 < a.K && g >= a.first[k + 1]) ++k;
        const int64_t i = g - a.first[k];
        const uint64_t view = walk_view(a.seed, k);
        int64_t v = clamp(walk_start(view, i, L, a.N), 0, a.N - 1);
        int64_t* out = a.walks ? a.walks + g * (L + 1) : nullptr;
        ns_mark(a, k, v);
        if (out) out[0] = v;
        for (int64_t t = 1; t <= L; ++t) {
            const int64_t s = clamp(a.lo[v], 0, a.E);
            const int64_t d = clamp(a.hi[v], s, a.E) - s;
            if (d > 0) {
                const int64_t place = clamp(walk_place(view, i, t, L, d), 0, d - 1);
                v = clamp(a.tgts[clamp(s + place, 0, a.E - 1)], 0, a.N - 1);
                ns_mark(a, k, v);
            }
            if (out) out[t] = v;
        }
    }
}

// drop, for the node mask only: word w of every view from the coins of nodes [64 w, 64 w + 64), a wave a word
__global__ __launch_bounds__(TILE) void k_ns_drop_bits(Ns a) {
    if (ns_failed(a)) return;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t waves = (int64_t)gridDim.x * (TILE / WAVE);
    for (int64_t w = (int64_t)blockIdx.x * (TILE / WAVE) + threadIdx.x / WAVE; w < a.W; w += waves) {
        const int64_t v = w * WAVE + lane;
        const uint64_t h = node_hash(v);
        for (int k = 0; k < a.K; ++k) {
            const unsigned long long b = __ballot(v < a.N && node_kept(node_view(a.seed, k), h, a.p[k]));
            if (lane == 0) a.bits[(int64_t)k * a.W + w] = b;
        }
    }
}

// the node mask, a byte a node, from the bitmap
__global__ __launch_bounds__(TILE) void k_ns_mask(Ns a) {
    if (ns_failed(a)) return;
    const int64_t total = (int64_t)a.K * a.N;
    for (int64_t j = (int64_t)blockIdx.x * TILE + threadIdx.x; j < total; j += (int64_t)gridDim.x * TILE) {
        const int64_t k = j / a.N, v = j - k * a.N;
        a.node_mask[j] = set_test(a.bits + k * a.W, v) ? 1 : 0;
    }
}

// ---------------------------------------------------------------- flip and compact: rlap_rowcompact_dev.h's passes with these predicates
// drop: a lane keeps the hashes of a row's two ids
struct NodeCoins {
    static constexpr bool MASK = false;
    struct Row { uint64_t a, b; };
    double p[MAX_VIEWS]; uint64_t seed;
    __device__ Row row(const rowcompact::Rows& c, int64_t e) const {
        const int64_t s = e < c.E ? c.src[e] : 0, d = e < c.E ? c.dst[e] : 0;
        return Row{node_hash(s), node_hash(d)};
    }
    __device__ uint64_t view(int k) const { return node_view(seed, k); }
    __device__ bool keep(int k, uint64_t view, const Row& r) const { return node_kept(view, r.a, p[k]) && node_kept(view, r.b, p[k]); }
};

// walk: a lane keeps the two ids, clamped into the bitmap; the per-view constant is the view's bitmap
struct InWalk {
    static constexpr bool MASK = false;
    struct Row { int64_t a, b; };
    int64_t N, W; const uint64_t* bits;
    __device__ Row row(const rowcompact::Rows& c, int64_t e) const {
        const int64_t s = e < c.E ? c.src[e] : 0, d = e < c.E ? c.dst[e] : 0;
        return Row{clamp(s, 0, N - 1), clamp(d, 0, N - 1)};
    }
    __device__ const uint64_t* view(int k) const { return bits + (int64_t)k * W; }
    __device__ bool keep(int, const uint64_t* view, const Row& r) const { return set_test(view, r.a) && set_test(view, r.b); }
};

struct Bufs {
    int32_t* words;
    int32_t *val, *perm, *lo, *hi, *tgts;
    uint32_t *key, *skey;
    uint64_t* bits;
    rowcompact::Scratch compact;
    void* sort_tmp; size_t sort_bytes;
};

size_t carve(Carve& C, int64_t E, int64_t N, int K, int scheme, bool node_mask, Bufs& B) {
    const bool csr = scheme == WALK;
    const int64_t nT = edgedrop::row_tiles(E);
    B.words = C.take<int32_t>(2 * W_WORDS64);
    B.key = C.take<uint32_t>(csr ? E : 0);
    B.skey = C.take<uint32_t>(csr ? E : 0);
    B.val = C.take<int32_t>(csr ? E : 0);
    B.perm = C.take<int32_t>(csr ? E : 0);
    B.tgts = C.take<int32_t>(csr ? E : 0);
    B.lo = C.take<int32_t>(csr ? N : 0);
    B.hi = C.take<int32_t>(csr ? N : 0);
    B.bits = C.take<uint64_t>(csr || node_mask ? (int64_t)K * set_words(N) : 0);
    rowcompact::carve(C, K, nT, B.compact);
    B.sort_bytes = csr ? rowcompact::list_sort_bytes(E, N) : 0;
    B.sort_tmp = C.take<char>((int64_t)B.sort_bytes);
    return C.off + 256;
}

}  // namespace

size_t node_sample_bytes(int64_t E, int64_t N, int K, int scheme, bool node_mask) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve(C, E, N, K, scheme, node_mask, B);
}

int node_sample_run(hipStream_t st, void* ws, size_t ws_bytes, const NodeSampleArgs& g, NodeSampleReport* rep) {
    *rep = NodeSampleReport{};
    const int64_t E = g.E, N = g.N, W = set_words(N), nT = edgedrop::row_tiles(E);
    const int K = g.K;
    const bool walk = g.scheme == WALK;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve(C, E, N, K, g.scheme, g.node_mask != nullptr, B) > ws_bytes) return RLAP_E_WORKSPACE;
    int64_t launches = 0;
    Ns a{};
    a.src = g.src; a.dst = g.dst; a.E = E; a.N = N; a.W = W; a.K = K;
    a.words = B.words; a.key = B.key; a.val = B.val; a.lo = B.lo; a.hi = B.hi; a.tgts = B.tgts;
    a.bits = B.bits; a.walk_length = g.walk_length; a.seed = g.seed; a.node_mask = g.node_mask; a.walks = g.walks;
    a.first[0] = 0;
    for (int k = 0; k < K; ++k) { a.p[k] = g.p[k]; a.first[k + 1] = a.first[k] + (walk ? g.seeds[k] : 0); }
    const int64_t walkers = a.first[K];
    RLAP_HIPCHK(hipMemsetAsync(B.words, 0, sizeof(int64_t) * W_WORDS64, st));
    // 1. the ids; walk: the lists of outgoing rows
    if (E > 0) RLAP_LAUNCH_COUNTED(k_ns_keys, ns_blocks(E), TILE, a, walk ? 1 : 0);
    if (walk && N > 0) {
        RLAP_HIPCHK(hipMemsetAsync(B.bits, 0, sizeof(uint64_t) * (size_t)((int64_t)K * W), st));
        // every node's outgoing rows in input order, their targets in list order
        const rowcompact::Lists l{E, N, B.words + W_ERR, B.key, B.val, B.skey, B.perm, B.lo, B.hi, g.dst, B.tgts, B.sort_tmp, B.sort_bytes};
        if (const int rc = rowcompact::build_lists(st, l, ns_blocks(E), launches)) return rc;
        // 2. the walks
        if (walkers > 0) RLAP_LAUNCH_COUNTED(k_ns_walk, ns_blocks(walkers), TILE, a);
    }
    // 3. the optional node mask
    if (g.node_mask && N > 0) {
        if (!walk) RLAP_LAUNCH_COUNTED(k_ns_drop_bits, capped_blocks(W, TILE / WAVE, NS_MAX_GRID), TILE, a);
        RLAP_LAUNCH_COUNTED(k_ns_mask, ns_blocks((int64_t)K * N), TILE, a);
    }
    // 4. flip and compact
    const rowcompact::Rows c{g.src, g.dst, g.w, E, nT, K, B.words + W_ERR, B.compact.counts, B.compact.offs, g.rows, g.cap, g.ptr, nullptr,
                             reinterpret_cast<int64_t*>(B.words) + W_TOTAL64};
    int rc;
    if (walk) {
        rc = rowcompact::run(st, c, InWalk{N, W, B.bits}, B.compact, nT > 0 && N > 0, launches);
    } else {
        NodeCoins p{};
        for (int k = 0; k < K; ++k) p.p[k] = g.p[k];
        p.seed = g.seed;
        rc = rowcompact::run(st, c, p, B.compact, nT > 0 && N > 0, launches);
    }
    if (rc != RLAP_OK) return rc;
    // 5. the error word and the total, read back once
    int64_t hw[W_WORDS64];
    RLAP_HIPCHK(hipMemcpyAsync(hw, B.words, sizeof(hw), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs = 1;
    rep->launches = launches;
    if (reinterpret_cast<const int32_t*>(hw)[W_ERR]) return RLAP_E_INDEX_RANGE;
    rep->rows_needed = hw[W_TOTAL64];
    if (hw[W_TOTAL64] < 0 || hw[W_TOTAL64] > (int64_t)K * E) return RLAP_E_INTERNAL;
    if (hw[W_TOTAL64] > g.cap) return RLAP_E_OUT_CAPACITY;
    return RLAP_OK;
}

}  // namespace rlap
