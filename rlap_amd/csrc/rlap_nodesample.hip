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
//   flip     the per-row kernels: pass A counts the kept rows per (view, tile of 2,048 rows) for all K views from one read of the
//            row's two ids, one scan gives the offsets and ptr, pass B writes [source, target, weight] at offset + rank (ballot and
//            population count within the wave, wave counts in LDS), rows in input order.  drop: the predicate is two node coins
//            recomputed in registers; walk: two bit tests in the view's bitmap.
//   One read-back: the error word and the row total.  No atomic on a float; LDS holds wave counts only.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_nodesample.h"
#include "rlap_snapshot.h"

namespace rlap {
namespace {

using namespace nodesample;

constexpr int64_t NS_MAX_GRID = 8192;                    // workgroups of a strided launch
constexpr int ROUNDS = ROW_TILE / TILE;                  // rows a lane flips
enum { W_ERR = 0, W_TOTAL64 = 1, W_WORDS64 = 2 };        // int32 word 0; the total is int64 word 1

inline unsigned ns_blocks(int64_t n) { return capped_blocks(n, TILE, NS_MAX_GRID); }

__device__ inline int64_t ns_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct Ns {
    const int64_t* src; const int64_t* dst; int64_t E, N, W;   // W: words of one view's bitmap
    int K;
    int32_t* words;
    uint32_t* key; int32_t* val; uint32_t* skey; int32_t* perm; int32_t* lo; int32_t* hi; int32_t* tgts;
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

// [lo[v], hi[v]) = the positions of source v among the sorted rows (both zeroed before); the targets in list order
__global__ __launch_bounds__(TILE) void k_ns_bounds(Ns a) {
    if (ns_failed(a)) return;
    for (int64_t p = (int64_t)blockIdx.x * TILE + threadIdx.x; p < a.E; p += (int64_t)gridDim.x * TILE) {
        const int64_t key = a.skey[p];
        a.tgts[p] = (int32_t)ns_clamp(a.dst[ns_clamp(a.perm[p], 0, a.E - 1)], 0, a.N - 1);
        if (key >= a.N) continue;
        if (p == 0 || a.skey[p - 1] != key) a.lo[key] = (int32_t)p;
        if (p == a.E - 1 || a.skey[p + 1] != key) a.hi[key] = (int32_t)(p + 1);
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
        int64_t v = ns_clamp(walk_start(view, i, L, a.N), 0, a.N - 1);
        int64_t* out = a.walks ? a.walks + g * (L + 1) : nullptr;
        ns_mark(a, k, v);
        if (out) out[0] = v;
        for (int64_t t = 1; t <= L; ++t) {
            const int64_t s = ns_clamp(a.lo[v], 0, a.E);
            const int64_t d = ns_clamp(a.hi[v], s, a.E) - s;
            if (d > 0) {
                const int64_t place = ns_clamp(walk_place(view, i, t, L, d), 0, d - 1);
                v = ns_clamp(a.tgts[ns_clamp(s + place, 0, a.E - 1)], 0, a.N - 1);
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

// ---------------------------------------------------------------- flip and compact
struct Flip {
    const int64_t* src; const int64_t* dst; const double* w; int64_t E, N, W, nT;   // nT: row tiles
    int K;
    double p[MAX_VIEWS]; uint64_t seed; const uint64_t* bits;
    const int32_t* words; int32_t* counts; const int64_t* offs;                     // [K * nT + 1], view-major
    double* rows; int64_t cap; int64_t* ptr;
};

// what a lane knows of its ROUNDS rows: drop: the hashes of the two ids; walk: the two ids, clamped into the bitmap
template <bool WALKS>
__device__ inline void flip_load(const Flip& f, int64_t base, uint64_t (&a)[ROUNDS], uint64_t (&b)[ROUNDS]) {
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
        const int64_t e = base + r * TILE + threadIdx.x;
        const int64_t s = e < f.E ? f.src[e] : 0, d = e < f.E ? f.dst[e] : 0;
        if (WALKS) {
            a[r] = (uint64_t)ns_clamp(s, 0, f.N - 1);
            b[r] = (uint64_t)ns_clamp(d, 0, f.N - 1);
        } else {
            a[r] = node_hash(s);
            b[r] = node_hash(d);
        }
    }
}

template <bool WALKS>
__device__ inline bool flip_keep(const Flip& f, int k, uint64_t view, uint64_t a, uint64_t b) {
    if (WALKS) {
        const uint64_t* bits = f.bits + (int64_t)k * f.W;
        return set_test(bits, (int64_t)a) && set_test(bits, (int64_t)b);
    }
    return node_kept(view, a, f.p[k]) && node_kept(view, b, f.p[k]);
}

// pass A: the kept rows of every (view, tile)
template <bool WALKS>
__global__ __launch_bounds__(TILE) void k_ns_count(Flip f) {
    __shared__ int wc[MAX_VIEWS][TILE / WAVE];
    if (f.words[W_ERR]) return;
    const int64_t base = (int64_t)blockIdx.x * ROW_TILE;
    uint64_t a[ROUNDS], b[ROUNDS];
    flip_load<WALKS>(f, base, a, b);
    for (int k = 0; k < f.K; ++k) {
        const uint64_t view = node_view(f.seed, k);
        int c = 0;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const bool keep = base + r * TILE + threadIdx.x < f.E && flip_keep<WALKS>(f, k, view, a[r], b[r]);
            c += __popcll(__ballot(keep));
        }
        if ((threadIdx.x & (WAVE - 1)) == 0) wc[k][threadIdx.x / WAVE] = c;
    }
    __syncthreads();
    if ((int)threadIdx.x < f.K) {
        const int k = threadIdx.x;
        f.counts[(int64_t)k * f.nT + blockIdx.x] = (wc[k][0] + wc[k][1]) + (wc[k][2] + wc[k][3]);
    }
}

// ptr[k] = the first row of view k; the total for the host
__global__ __launch_bounds__(WAVE) void k_ns_ptr(Flip f, int32_t* words) {
    const int k = threadIdx.x;
    if (k <= f.K) f.ptr[k] = f.offs[(int64_t)k * f.nT];
    if (k == 0) reinterpret_cast<int64_t*>(words)[W_TOTAL64] = f.offs[(int64_t)f.K * f.nT];
}

// pass B: the predicate again, the rows at offset + rank
template <bool WALKS>
__global__ __launch_bounds__(TILE) void k_ns_write(Flip f) {
    __shared__ int wc[ROUNDS][TILE / WAVE];
    if (f.words[W_ERR]) return;
    if (f.offs[(int64_t)f.K * f.nT] > f.cap) return;   // (too little room: nothing is written)
    const int64_t base = (int64_t)blockIdx.x * ROW_TILE;
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    uint64_t a[ROUNDS], b[ROUNDS];
    flip_load<WALKS>(f, base, a, b);
    for (int k = 0; k < f.K; ++k) {
        const uint64_t view = node_view(f.seed, k);
        const int64_t off = f.offs[(int64_t)k * f.nT + blockIdx.x], end = f.offs[(int64_t)k * f.nT + blockIdx.x + 1];
        unsigned kept = 0;
        int rank[ROUNDS];
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int64_t e = base + r * TILE + threadIdx.x;
            const bool keep = e < f.E && flip_keep<WALKS>(f, k, view, a[r], b[r]);
            const unsigned long long bal = __ballot(keep);
            rank[r] = __popcll(bal & ((1ull << lane) - 1ull));
            kept |= keep ? 1u << r : 0u;
            if (lane == 0) wc[r][wave] = __popcll(bal);
        }
        __syncthreads();
        int pre = 0;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
#pragma unroll
            for (int w = 0; w < TILE / WAVE; ++w) {
                if (w == wave) rank[r] += pre;
                pre += wc[r][w];
            }
        }
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const int64_t e = base + r * TILE + threadIdx.x;
            const int64_t pos = off + rank[r];
            if (!(kept >> r & 1u) || pos >= end || pos >= f.cap) continue;
            double* __restrict__ o = f.rows + 3 * pos;
            o[0] = (double)f.src[e]; o[1] = (double)f.dst[e]; o[2] = f.w ? f.w[e] : 1.0;
        }
        __syncthreads();   // (wc is rewritten by the next view)
    }
}

struct Bufs {
    int32_t* words;
    int32_t *val, *perm, *lo, *hi, *tgts, *counts;
    uint32_t *key, *skey;
    uint64_t* bits;
    int64_t* offs;
    void* scan_tmp; size_t scan_bytes;
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
    B.counts = C.take<int32_t>((int64_t)K * nT + 1);
    B.offs = C.take<int64_t>((int64_t)K * nT + 1);
    B.scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, B.scan_bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)((int64_t)K * nT + 1),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    B.scan_tmp = C.take<char>((int64_t)B.scan_bytes);
    B.sort_bytes = 0;
    if (csr)
        (void)rocprim::radix_sort_pairs(nullptr, B.sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int32_t*)nullptr,
                                        (int32_t*)nullptr, (size_t)std::max<int64_t>(E, 1), 0u, edgeplan::key_bits(N), (hipStream_t)0);
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
#define NS_LAUNCH(kernel, grid, block, ...)                                            \
    do {                                                                               \
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);       \
        RLAP_HIPCHK(hipGetLastError());                                                \
        ++launches;                                                                    \
    } while (0)
    Ns a{};
    a.src = g.src; a.dst = g.dst; a.E = E; a.N = N; a.W = W; a.K = K;
    a.words = B.words; a.key = B.key; a.val = B.val; a.skey = B.skey; a.perm = B.perm; a.lo = B.lo; a.hi = B.hi; a.tgts = B.tgts;
    a.bits = B.bits; a.walk_length = g.walk_length; a.seed = g.seed; a.node_mask = g.node_mask; a.walks = g.walks;
    a.first[0] = 0;
    for (int k = 0; k < K; ++k) { a.p[k] = g.p[k]; a.first[k + 1] = a.first[k] + (walk ? g.seeds[k] : 0); }
    const int64_t walkers = a.first[K];
    RLAP_HIPCHK(hipMemsetAsync(B.words, 0, sizeof(int64_t) * W_WORDS64, st));
    // 1. the ids; walk: the lists of outgoing rows
    if (E > 0) NS_LAUNCH(k_ns_keys, ns_blocks(E), TILE, a, walk ? 1 : 0);
    if (walk && N > 0) {
        RLAP_HIPCHK(hipMemsetAsync(B.lo, 0, sizeof(int32_t) * (size_t)N, st));
        RLAP_HIPCHK(hipMemsetAsync(B.hi, 0, sizeof(int32_t) * (size_t)N, st));
        RLAP_HIPCHK(hipMemsetAsync(B.bits, 0, sizeof(uint64_t) * (size_t)((int64_t)K * W), st));
        if (E > 0) {
            size_t sb = B.sort_bytes;
            RLAP_HIPCHK(rocprim::radix_sort_pairs(B.sort_tmp, sb, (const uint32_t*)B.key, B.skey, (const int32_t*)B.val, B.perm, (size_t)E, 0u,
                                                edgeplan::key_bits(N), st));
            NS_LAUNCH(k_ns_bounds, ns_blocks(E), TILE, a);
        }
        // 2. the walks
        if (walkers > 0) NS_LAUNCH(k_ns_walk, ns_blocks(walkers), TILE, a);
    }
    // 3. the optional node mask
    if (g.node_mask && N > 0) {
        if (!walk) NS_LAUNCH(k_ns_drop_bits, capped_blocks(W, TILE / WAVE, NS_MAX_GRID), TILE, a);
        NS_LAUNCH(k_ns_mask, ns_blocks((int64_t)K * N), TILE, a);
    }
    // 4. flip and compact
    Flip f{};
    f.src = g.src; f.dst = g.dst; f.w = g.w; f.E = E; f.N = N; f.W = W; f.nT = nT;
    f.K = K;
    for (int k = 0; k < K; ++k) f.p[k] = g.p[k];
    f.seed = g.seed; f.bits = B.bits;
    f.words = B.words; f.counts = B.counts; f.offs = B.offs;
    f.rows = g.rows; f.cap = g.cap; f.ptr = g.ptr;
    RLAP_HIPCHK(hipMemsetAsync(B.counts, 0, sizeof(int32_t) * (size_t)((int64_t)K * nT + 1), st));
    if (nT > 0 && N > 0) {
        if (walk) NS_LAUNCH(k_ns_count<true>, (unsigned)nT, TILE, f);
        else NS_LAUNCH(k_ns_count<false>, (unsigned)nT, TILE, f);
    }
    size_t cb = B.scan_bytes;
    RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.counts, B.offs, (int64_t)0, (size_t)((int64_t)K * nT + 1), rocprim::plus<int64_t>(), st));
    NS_LAUNCH(k_ns_ptr, 1, WAVE, f, B.words);
    if (nT > 0 && N > 0) {
        if (walk) NS_LAUNCH(k_ns_write<true>, (unsigned)nT, TILE, f);
        else NS_LAUNCH(k_ns_write<false>, (unsigned)nT, TILE, f);
    }
#undef NS_LAUNCH
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
