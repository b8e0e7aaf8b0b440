// rlap_edgeadd.hip -- edge adding, K views a call (rlap_edge_add).  The rules -- the coin, the draw, the key of a pair,
// the tie rule of the merge and the weight -- are rlap_edgeadd.h's.  A translation unit of its own.
//
//   keys     one pass over the rows: both ids checked (a row that fails raises the error word; every later kernel returns on a raised
//            word), the 64-bit key (source << b) | target and the row number written, a word raised where a key is below the one
//            before it.
//   draws    one lane per (view, added row): the key of the drawn pair, the view number above it when one sort serves all views;
//            the optional `added` pairs from the same lane.  rocPRIM sorts the keys alone -- every added row weighs 1.0 -- once
//            for all views or once a view; a head-flag scan and one lane per run leave each view's distinct keys and their counts
//            (list B_k).
//   input    once a call: the distinct keys of the input and the sum of each one's rows in input order (list A): head flags, a
//            scan, one lane per run.  The host cannot know whether the keys ascend before it has asked, so this part and the merge
//            are first enqueued for ascending keys, every kernel of them returning on the raised word.  Behind them, and returning
//            unless the word is raised, a set of the input's keys (open addressing, integer compare-and-swap) gives the distinct
//            keys and, probed with every key of B_k, each view's rows: ptr and the row total without a sort.  The one read-back
//            holds the error word, the word and the total.  Only if the keys did not ascend, rocPRIM's stable radix sort of
//            (key, row) runs -- of the keys alone for an input without weights, whose sums are run lengths -- and the part is
//            enqueued again on its result: the rows follow in stream order, and nothing more is read back.
//   merge    a merge-path merge of A with B_k, a workgroup per (view, ROW_TILE merged positions): the tile's two ends are found by a
//            binary search along their diagonals, its slices of A and B_k staged in LDS (one array of ROW_TILE keys: the slices'
//            lengths add up to the tile), every lane finds its own start in LDS and walks PER_LANE positions, A first on ties.  A
//            position is a head if its key differs from the one before it in merged order (for a tile's first position:
//            max(A[a0 - 1], B[b0 - 1]) from memory), so a run that crosses a tile border is flagged once.  Pass 1 counts the heads
//            of a tile, one scan gives the offsets and ptr, pass 2 walks again, stages (key, s_in + c_add) in LDS at the row's rank
//            in the tile and the workgroup writes [source, target, weight] from offset on, a lane a float64 of consecutive addresses.
//   Without coalesce: the range check, a copy of the rows and the draws written as rows.
//   No atomic on a float; the two integer words (error, not ascending) are raised by an atomic OR only where they are not seen raised.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_edgeadd.h"
#include "rlap_rowcompact_dev.h"
#include "rlap_snapshot.h"

namespace rlap {
namespace {

using namespace edgeadd;
using rowcompact::clamp;
using rowcompact::scan_tmp_bytes;
using rowcompact::store_row;

constexpr int64_t EA_MAX_GRID = 8192;                            // workgroups of a strided launch
enum { W_ERR = 0, W_UNSORTED = 1 };                              // int32 words
enum { W_NA64 = 1, W_TOTAL64 = 2, W_HOST64 = 3 };                // int64 words the host reads back ...
enum { W_VIEW64 = W_HOST64, W_WORDS64 = W_HOST64 + MAX_VIEWS };  // ... and a counter a view: its added keys that the input does not hold
constexpr uint64_t EMPTY_SLOT = ~(uint64_t)0;                    // (no key: bit 63 of every key is clear)

inline unsigned ea_blocks(int64_t n) { return capped_blocks(n, TILE, EA_MAX_GRID); }

struct Ea {
    const int64_t* src; const int64_t* dst; const double* w; int64_t E, N;
    int K, one;                                   // one: the view number rides above the key
    unsigned b;
    int32_t* words;
    uint64_t* kin; int32_t* vin;                  // [E] keys and row numbers in input order
    uint64_t* bin; const uint64_t* bs;            // [first[K]] the draws' keys as drawn, and sorted inside each view
    int32_t* flag_b; const int64_t* pos_b;        // [first[K] + 1]
    uint64_t* bkey; int32_t* bcnt;                // [first[K]] list B of every view, view-major
    uint64_t* table; int64_t slots;               // the set of the input's keys, open addressing (an input whose keys do not ascend)
    int64_t first[MAX_VIEWS + 1]; uint64_t seed;  // view k owns added rows [first[k], first[k + 1])
    double* rows; int64_t cap; int64_t* ptr; int64_t* added; int64_t* aptr;
};

__device__ inline bool ea_failed(const int32_t* words) { return words[W_ERR] != 0; }

__device__ inline int ea_view_of(const Ea& a, int64_t g) {
    int k = 0;
    while (k + 1 < a.K && g >= a.first[k + 1]) ++k;
    return k;
}

// raises a word: an atomic only where it is not seen raised (half the rows of a shuffled input would otherwise queue on one address)
__device__ inline void ea_raise(int32_t* word) {
    if (__atomic_load_n(word, __ATOMIC_RELAXED) == 0) atomicOr(word, 1);
}

__device__ inline bool ea_in_range(const Ea& a, int64_t s, int64_t d) { return s >= 0 && s < a.N && d >= 0 && d < a.N; }

__global__ __launch_bounds__(TILE) void k_ea_keys(Ea a, int keys) {
    for (int64_t e = (int64_t)blockIdx.x * TILE + threadIdx.x; e < a.E; e += (int64_t)gridDim.x * TILE) {
        const int64_t s = a.src[e], d = a.dst[e];
        const bool ok = ea_in_range(a, s, d);
        if (!ok) ea_raise(&a.words[W_ERR]);
        if (!keys) continue;
        const uint64_t key = ok ? pair_key(s, d, a.b) : 0;
        a.kin[e] = key;
        a.vin[e] = (int32_t)e;
        if (e > 0) {
            const int64_t sp = a.src[e - 1], dp = a.dst[e - 1];
            if (ea_in_range(a, sp, dp) && pair_key(sp, dp, a.b) > key) ea_raise(&a.words[W_UNSORTED]);
        }
    }
}

// one lane per (view, added row); rows: the uncoalesced call, which writes the draws as rows behind the view's copy of the input
__global__ __launch_bounds__(TILE) void k_ea_draw(Ea a, int as_rows) {
    if (as_rows && ea_failed(a.words)) return;
    const int64_t total = a.first[a.K];
    for (int64_t g = (int64_t)blockIdx.x * TILE + threadIdx.x; g < total; g += (int64_t)gridDim.x * TILE) {
        const int k = ea_view_of(a, g);
        const int64_t i = g - a.first[k];
        const uint64_t view = add_view(a.seed, k);
        const int64_t s = clamp(draw(view, i, 0, a.N), 0, a.N - 1), t = clamp(draw(view, i, 1, a.N), 0, a.N - 1);
        if (a.added) { a.added[2 * g] = s; a.added[2 * g + 1] = t; }
        if (as_rows) {
            const int64_t pos = (int64_t)(k + 1) * a.E + g;
            if (pos < a.cap) store_row(a.rows, pos, (double)s, (double)t, 1.0);
        } else {
            a.bin[g] = pair_key(s, t, a.b) | (a.one ? (uint64_t)k << (2 * a.b) : (uint64_t)0);
        }
    }
}

// the uncoalesced call: view k's copy of the rows, in input order
__global__ __launch_bounds__(TILE) void k_ea_copy(Ea a) {
    if (ea_failed(a.words)) return;
    const int64_t total = (int64_t)a.K * a.E;
    for (int64_t j = (int64_t)blockIdx.x * TILE + threadIdx.x; j < total; j += (int64_t)gridDim.x * TILE) {
        const int64_t k = j / a.E, e = j - k * a.E, pos = j + a.first[k];
        if (pos >= a.cap) continue;
        store_row(a.rows, pos, (double)a.src[e], (double)a.dst[e], a.w ? a.w[e] : 1.0);
    }
}
__global__ __launch_bounds__(WAVE) void k_ea_plain_ptr(Ea a) {
    const int k = threadIdx.x;
    if (k > a.K) return;
    a.ptr[k] = (int64_t)k * a.E + a.first[k];
    if (a.aptr) a.aptr[k] = a.first[k];
}

// ---------------------------------------------------------------- list B: the distinct keys of a view's added rows and their counts
__global__ __launch_bounds__(TILE) void k_ea_heads_b(Ea a) {
    const int64_t total = a.first[a.K];
    for (int64_t g = (int64_t)blockIdx.x * TILE + threadIdx.x; g <= total; g += (int64_t)gridDim.x * TILE) {
        if (g == total) { a.flag_b[g] = 0; continue; }
        a.flag_b[g] = g == a.first[ea_view_of(a, g)] || a.bs[g] != a.bs[g - 1];
    }
}
__global__ __launch_bounds__(TILE) void k_ea_runs_b(Ea a) {
    const int64_t total = a.first[a.K];
    const uint64_t mask = ((uint64_t)1 << (2 * a.b)) - 1;
    for (int64_t g = (int64_t)blockIdx.x * TILE + threadIdx.x; g < total; g += (int64_t)gridDim.x * TILE) {
        if (!a.flag_b[g]) continue;
        const int64_t end = a.first[ea_view_of(a, g) + 1], p = clamp(a.pos_b[g], 0, total - 1);
        const uint64_t key = a.bs[g];
        int64_t j = g + 1;
        while (j < end && a.bs[j] == key) ++j;
        a.bkey[p] = key & mask;
        a.bcnt[p] = (int32_t)(j - g);
    }
}

// ---------------------------------------------------------------- the row total of an input whose keys do not ascend, without its sort
// The host reads back once, and the total must be in that read-back: rows of view k = n_a + (the keys of B_k that A does not hold).
// Both counts come from a set of the input's keys (open addressing, linear probing, integer compare-and-swap: which lane wins a slot
// changes no count).  Every kernel here returns unless the not-ascending word is raised.
__device__ inline bool hash_off(const Ea& a) { return a.words[W_ERR] != 0 || a.words[W_UNSORTED] == 0; }
__device__ inline int64_t hash_home(const Ea& a, uint64_t key) { return (int64_t)(mix64(key) % (uint64_t)a.slots); }

// adds a lane's count to an int64 word: the wave's sum, one integer atomic a wave
__device__ inline void ea_count(int32_t* words, int word, int64_t mine) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o, WAVE);
    if ((threadIdx.x & (WAVE - 1)) == 0 && mine != 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(words) + word, (unsigned long long)mine);
}

__global__ __launch_bounds__(TILE) void k_ea_hash_clear(Ea a) {
    if (hash_off(a)) return;
    for (int64_t i = (int64_t)blockIdx.x * TILE + threadIdx.x; i < a.slots; i += (int64_t)gridDim.x * TILE) a.table[i] = EMPTY_SLOT;
}

__global__ __launch_bounds__(TILE) void k_ea_hash_insert(Ea a) {
    if (hash_off(a)) return;
    int64_t fresh = 0;
    for (int64_t e = (int64_t)blockIdx.x * TILE + threadIdx.x; e < a.E; e += (int64_t)gridDim.x * TILE) {
        const uint64_t key = a.kin[e];
        int64_t h = hash_home(a, key);
        for (int64_t tries = 0; tries < a.slots; ++tries) {
            const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(a.table) + h, (unsigned long long)EMPTY_SLOT, (unsigned long long)key);
            if (old == EMPTY_SLOT) { ++fresh; break; }
            if (old == key) break;
            h = h + 1 == a.slots ? 0 : h + 1;
        }
    }
    ea_count(a.words, W_NA64, fresh);
}

// every head of the sorted draws: a key of B_k; counted for its view unless the input holds it
__global__ __launch_bounds__(TILE) void k_ea_hash_probe(Ea a) {
    if (hash_off(a)) return;
    const int64_t total = a.first[a.K];
    const uint64_t mask = ((uint64_t)1 << (2 * a.b)) - 1;
    for (int k = 0; k < a.K; ++k) {
        int64_t fresh = 0;
        for (int64_t g = a.first[k] + (int64_t)blockIdx.x * TILE + threadIdx.x; g < a.first[k + 1] && g < total; g += (int64_t)gridDim.x * TILE) {
            if (!a.flag_b[g]) continue;
            const uint64_t key = a.bs[g] & mask;
            bool held = false;
            if (a.slots > 0) {
                int64_t h = hash_home(a, key);
                for (int64_t tries = 0; tries < a.slots; ++tries) {
                    const uint64_t at = a.table[h];
                    if (at == key) { held = true; break; }
                    if (at == EMPTY_SLOT) break;
                    h = h + 1 == a.slots ? 0 : h + 1;
                }
            }
            fresh += held ? 0 : 1;
        }
        ea_count(a.words, W_VIEW64 + k, fresh);
    }
}

// ptr, aptr and the total from the counts
__global__ __launch_bounds__(WAVE) void k_ea_hash_ptr(Ea a) {
    if (hash_off(a) || threadIdx.x != 0) return;
    const int64_t* w64 = reinterpret_cast<const int64_t*>(a.words);
    int64_t at = 0;
    for (int k = 0; k < a.K; ++k) {
        a.ptr[k] = at;
        if (a.aptr) a.aptr[k] = a.first[k];
        at += w64[W_NA64] + w64[W_VIEW64 + k];
    }
    a.ptr[a.K] = at;
    if (a.aptr) a.aptr[a.K] = a.first[a.K];
    reinterpret_cast<int64_t*>(a.words)[W_TOTAL64] = at;
}

// ---------------------------------------------------------------- list A and the merge: enqueued for keys that ascend
struct Tail {
    const double* w; int64_t E;
    const uint64_t* key; const int32_t* perm;     // [E] the input's keys ascending and the row of each (null: the rows as they stand)
    int gate;                                     // return where the input's keys did not ascend
    int32_t* words;
    int32_t* flag_a; const int64_t* pos_a;        // [E + 1]
    uint64_t* akey; double* asum;                 // [E] list A
    const uint64_t* bkey; const int32_t* bcnt; const int64_t* pos_b;
    int64_t first[MAX_VIEWS + 1]; int K; unsigned b;
    int64_t nT;                                   // tiles of a view in the grid
    int32_t* counts; const int64_t* offs;         // [K * nT + 1], view-major
    double* rows; int64_t cap; int64_t* ptr; int64_t* aptr;
};

__device__ inline bool tail_off(const Tail& t) { return t.words[W_ERR] != 0 || (t.gate && t.words[W_UNSORTED] != 0); }

__global__ __launch_bounds__(TILE) void k_ea_heads_a(Tail t) {
    if (tail_off(t)) return;
    for (int64_t e = (int64_t)blockIdx.x * TILE + threadIdx.x; e <= t.E; e += (int64_t)gridDim.x * TILE)
        t.flag_a[e] = e < t.E && (e == 0 || t.key[e] != t.key[e - 1]);
}

// one lane per run of equal keys: the rows of the run are in input order (the sort is stable), and so is the sum
__global__ __launch_bounds__(TILE) void k_ea_runs_a(Tail t) {
    if (tail_off(t)) return;
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int64_t*>(t.words)[W_NA64] = t.pos_a[t.E];
    for (int64_t e = (int64_t)blockIdx.x * TILE + threadIdx.x; e < t.E; e += (int64_t)gridDim.x * TILE) {
        if (!t.flag_a[e]) continue;
        const uint64_t key = t.key[e];
        const int64_t p = clamp(t.pos_a[e], 0, t.E - 1);
        double s = 0.0;
        for (int64_t j = e; j < t.E && t.key[j] == key; ++j) {
            const int64_t row = t.perm ? clamp(t.perm[j], 0, t.E - 1) : j;
            s = run_add(s, t.w ? t.w[row] : 1.0);
        }
        t.akey[p] = key;
        t.asum[p] = s;
    }
}

// a lane's PER_LANE merged positions from (ai, bi) on, A first on ties: visit(key, from A, index in the slice, head)
template <class Visit>
__device__ inline void lane_walk(const uint64_t* sA, int la, const uint64_t* sB, int lb, int ai, int bi, bool has_prev, uint64_t prev, Visit visit) {
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        if (ai >= la && bi >= lb) break;
        const bool from_a = ai < la && (bi >= lb || takes_a(sA[ai], sB[bi]));
        const uint64_t key = from_a ? sA[ai] : sB[bi];
        visit(key, from_a, from_a ? ai : bi, bi, !has_prev || key != prev);
        if (from_a) ++ai; else ++bi;
        prev = key;
        has_prev = true;
    }
}

template <bool WRITE>
__global__ __launch_bounds__(TILE) void k_ea_merge(Tail t) {
    __shared__ uint64_t keys[ROW_TILE];
    __shared__ int64_t ends[2];
    __shared__ int wsum[TILE / WAVE];
    __shared__ uint64_t okey[WRITE ? ROW_TILE : 1];   // pass 2: the tile's rows by rank, key and weight
    __shared__ double ow[WRITE ? ROW_TILE : 1];
    if (tail_off(t)) return;
    const int k = blockIdx.y;
    const int64_t slot = (int64_t)k * t.nT + blockIdx.x;
    if (WRITE && t.offs[(int64_t)t.K * t.nT] > t.cap) return;   // (too little room: nothing is written)
    const int64_t addk = t.first[k + 1] - t.first[k];
    const int64_t na = clamp(reinterpret_cast<const int64_t*>(t.words)[W_NA64], 0, t.E);
    const int64_t bfirst = clamp(t.pos_b[t.first[k]], 0, t.first[t.K]);
    const int64_t nb = clamp(t.pos_b[t.first[k + 1]] - bfirst, 0, addk);
    const uint64_t* __restrict__ A = t.akey;
    const uint64_t* __restrict__ B = t.bkey + bfirst;
    const int64_t L = na + nb;
    const int64_t d0 = std::min<int64_t>((int64_t)blockIdx.x * ROW_TILE, L), d1 = std::min<int64_t>(d0 + ROW_TILE, L);
    if (d0 >= d1) return;                                        // (a tile past the view's end: its count stays 0)
    if (threadIdx.x < 2)
        ends[threadIdx.x] = merge_split(threadIdx.x ? d1 : d0, na, nb, [&](int64_t i) { return A[i]; }, [&](int64_t i) { return B[i]; });
    __syncthreads();
    const int64_t a0 = ends[0], a1 = ends[1], b0 = d0 - a0, b1 = d1 - a1;
    const int la = (int)clamp(a1 - a0, 0, ROW_TILE), lb = (int)clamp(b1 - b0, 0, ROW_TILE - la), n = la + lb;
    for (int i = threadIdx.x; i < n; i += TILE) keys[i] = i < la ? A[a0 + i] : B[b0 + (i - la)];
    __syncthreads();
    const uint64_t* sA = keys;
    const uint64_t* sB = keys + la;
    const int dd = std::min<int>((int)threadIdx.x * PER_LANE, n);
    const int ai = (int)merge_split(dd, la, lb, [&](int64_t i) { return sA[i]; }, [&](int64_t i) { return sB[i]; }), bi = dd - ai;
    bool has_prev = false;
    uint64_t prev = 0;
    if (dd > 0) {
        has_prev = true;
        prev = ai > 0 ? sA[ai - 1] : 0;
        if (bi > 0 && (ai == 0 || sB[bi - 1] > prev)) prev = sB[bi - 1];
    } else if (d0 > 0) {
        has_prev = true;
        prev = a0 > 0 ? A[a0 - 1] : 0;
        if (b0 > 0 && (a0 == 0 || B[b0 - 1] > prev)) prev = B[b0 - 1];
    }
    int heads = 0;
    lane_walk(sA, la, sB, lb, ai, bi, has_prev, prev, [&](uint64_t, bool, int, int, bool head) { heads += head ? 1 : 0; });
    // the lane's rank among the tile's heads
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    int incl = heads;
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += up;
    }
    if (lane == WAVE - 1) wsum[wave] = incl;
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0) t.counts[slot] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        return;
    }
    int rank = incl - heads;
#pragma unroll
    for (int w = 0; w < TILE / WAVE; ++w)
        if (w < wave) rank += wsum[w];
    const int64_t off = t.offs[slot], end = t.offs[slot + 1];
    const double* __restrict__ asum = t.asum;
    const int32_t* __restrict__ bcnt = t.bcnt + bfirst;
    const unsigned b = t.b;
    // the tile's rows are staged in LDS by rank, then written by the whole workgroup, a lane a float64 of consecutive addresses
    lane_walk(sA, la, sB, lb, ai, bi, has_prev, prev, [&](uint64_t key, bool from_a, int idx, int bcur, bool head) {
        if (!head) return;
        const int at = rank;
        ++rank;
        if (at >= ROW_TILE) return;
        double s_in = 0.0;
        int64_t c_add;
        if (from_a) {
            // the pair's added rows, if any, are B's next entry: every smaller key of B is merged by now, and of a tie A's comes first
            const int64_t bg = b0 + bcur;
            s_in = asum[a0 + idx];
            c_add = bg < nb && B[bg] == key ? bcnt[bg] : 0;
        } else {
            c_add = bcnt[b0 + idx];
        }
        okey[at] = key;
        ow[at] = weight(s_in, c_add);
    });
    __syncthreads();
    const int tile_heads = std::min<int>((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]), ROW_TILE);
    const int64_t room = std::min<int64_t>(end, t.cap) - off;
    const int rows_out = (int)clamp(room, 0, tile_heads);
    double* __restrict__ o = t.rows + 3 * off;
    for (int i = threadIdx.x; i < 3 * rows_out; i += TILE) {
        const int row = i / 3, c = i - 3 * row;
        o[i] = c == 2 ? ow[row] : (double)(c == 0 ? key_source(okey[row], b) : key_target(okey[row], b));
    }
}

// ptr[k] = the first row of view k; the total for the host
__global__ __launch_bounds__(WAVE) void k_ea_ptr(Tail t) {
    if (tail_off(t)) return;
    const int k = threadIdx.x;
    if (k <= t.K) {
        t.ptr[k] = t.offs[(int64_t)k * t.nT];
        if (t.aptr) t.aptr[k] = t.first[k];
    }
    if (k == 0) reinterpret_cast<int64_t*>(t.words)[W_TOTAL64] = t.offs[(int64_t)t.K * t.nT];
}

struct Bufs {
    int32_t* words;
    uint64_t *kin, *ks, *bin, *bs, *akey, *bkey, *table;
    int32_t *vin, *perm, *flag_a, *flag_b, *bcnt, *counts;
    int64_t *pos_a, *pos_b, *offs;
    double* asum;
    void* scan_tmp; size_t scan_bytes;
    void* sort_tmp; size_t sort_bytes;
};

struct Shape { int64_t added, max_add, nT; };

Shape shape_of(int64_t E, int K, const int64_t* num_add) {
    Shape s{0, 0, 1};
    for (int k = 0; k < K; ++k) { s.added += num_add[k]; s.max_add = std::max(s.max_add, num_add[k]); }
    s.nT = std::max<int64_t>(1, (E + s.max_add + ROW_TILE - 1) / ROW_TILE);
    return s;
}

size_t carve(Carve& C, int64_t E, int64_t N, int K, const int64_t* num_add, bool coalesce, Bufs& B) {
    const Shape s = shape_of(E, K, num_add);
    const int64_t e = coalesce ? E : 0, g = coalesce ? s.added : 0, slots = coalesce ? (int64_t)K * s.nT + 1 : 0;
    B.words = C.take<int32_t>(2 * W_WORDS64);
    B.kin = C.take<uint64_t>(e); B.ks = C.take<uint64_t>(e); B.akey = C.take<uint64_t>(e); B.asum = C.take<double>(e);
    B.vin = C.take<int32_t>(e); B.perm = C.take<int32_t>(e);
    B.flag_a = C.take<int32_t>(coalesce ? e + 1 : 0); B.pos_a = C.take<int64_t>(coalesce ? e + 1 : 0);
    B.bin = C.take<uint64_t>(g); B.bs = C.take<uint64_t>(g); B.bkey = C.take<uint64_t>(g); B.bcnt = C.take<int32_t>(g);
    B.flag_b = C.take<int32_t>(coalesce ? g + 1 : 0); B.pos_b = C.take<int64_t>(coalesce ? g + 1 : 0);
    B.counts = C.take<int32_t>(slots); B.offs = C.take<int64_t>(slots);
    B.table = C.take<uint64_t>(2 * e);   // (at most half full)
    B.scan_bytes = B.sort_bytes = 0;
    if (coalesce) {
        B.scan_bytes = std::max(scan_tmp_bytes(e + 1), std::max(scan_tmp_bytes(g + 1), scan_tmp_bytes(slots)));
        size_t pairs = 0, keys = 0;
        (void)rocprim::radix_sort_pairs(nullptr, pairs, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const int32_t*)nullptr, (int32_t*)nullptr,
                                        (size_t)std::max<int64_t>(e, 1), 0u, key_width(N), (hipStream_t)0);
        const bool one = one_sort(N, K);
        (void)rocprim::radix_sort_keys(nullptr, keys, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)std::max<int64_t>(one ? g : s.max_add, 1), 0u,
                                       key_width(N) + (one ? view_bits(K) : 0u), (hipStream_t)0);
        B.sort_bytes = std::max(pairs, keys);
        (void)rocprim::radix_sort_keys(nullptr, keys, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)std::max<int64_t>(e, 1), 0u, key_width(N),
                                       (hipStream_t)0);   // (the input without weights: its keys alone)
        B.sort_bytes = std::max(B.sort_bytes, keys);
    }
    B.scan_tmp = C.take<char>((int64_t)B.scan_bytes);
    B.sort_tmp = C.take<char>((int64_t)B.sort_bytes);
    return C.off + 256;
}

}  // namespace

size_t edge_add_bytes(int64_t E, int64_t N, int K, const int64_t* num_add, bool coalesce) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve(C, E, N, K, num_add, coalesce, B);
}

int edge_add_run(hipStream_t st, void* ws, size_t ws_bytes, const EdgeAddArgs& g, EdgeAddReport* rep) {
    *rep = EdgeAddReport{};
    const int64_t E = g.E, N = g.N;
    const int K = g.K;
    const Shape sh = shape_of(E, K, g.num_add);
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve(C, E, N, K, g.num_add, g.coalesce != 0, B) > ws_bytes) return RLAP_E_WORKSPACE;
    int64_t launches = 0;
    int32_t sorts = 0;
    Ea a{};
    a.src = g.src; a.dst = g.dst; a.w = g.w; a.E = E; a.N = N; a.K = K; a.b = id_bits(N); a.one = one_sort(N, K) ? 1 : 0;
    a.words = B.words; a.kin = B.kin; a.vin = B.vin; a.bin = B.bin; a.bs = B.bs; a.flag_b = B.flag_b; a.pos_b = B.pos_b;
    a.bkey = B.bkey; a.bcnt = B.bcnt; a.table = B.table; a.slots = g.coalesce ? 2 * E : 0; a.seed = g.seed;
    a.first[0] = 0;
    for (int k = 0; k < K; ++k) a.first[k + 1] = a.first[k] + g.num_add[k];
    a.rows = g.rows; a.cap = g.cap; a.ptr = g.ptr; a.added = g.added; a.aptr = g.aptr;
    rep->added = sh.added;
    RLAP_HIPCHK(hipMemsetAsync(B.words, 0, sizeof(int64_t) * W_WORDS64, st));
    int64_t hw[W_HOST64];
    const int32_t* h32 = reinterpret_cast<const int32_t*>(hw);
    if (!g.coalesce) {
        // the range check, the K copies of the rows and the draws behind them; the total is the host's to know
        const int64_t total = (int64_t)K * E + sh.added;
        rep->rows_needed = total;
        if (E > 0) RLAP_LAUNCH_COUNTED(k_ea_keys, dim3(ea_blocks(E)), TILE, a, 0);
        if (total <= g.cap) {
            if (E > 0) RLAP_LAUNCH_COUNTED(k_ea_copy, dim3(ea_blocks((int64_t)K * E)), TILE, a);
            if (sh.added > 0) RLAP_LAUNCH_COUNTED(k_ea_draw, dim3(ea_blocks(sh.added)), TILE, a, 1);
            RLAP_LAUNCH_COUNTED(k_ea_plain_ptr, dim3(1), WAVE, a);
        }
        RLAP_HIPCHK(hipMemcpyAsync(hw, B.words, sizeof(hw), hipMemcpyDeviceToHost, st));
        RLAP_HIPCHK(hipStreamSynchronize(st));
        rep->host_syncs = 1;
        rep->launches = launches;
        if (h32[W_ERR]) { rep->rows_needed = 0; return RLAP_E_INDEX_RANGE; }
        return total > g.cap ? RLAP_E_OUT_CAPACITY : RLAP_OK;
    }
    // 1. the input's keys; 2. the draws, their sort and list B of every view
    if (E > 0) RLAP_LAUNCH_COUNTED(k_ea_keys, dim3(ea_blocks(E)), TILE, a, 1);
    if (sh.added > 0) {
        RLAP_LAUNCH_COUNTED(k_ea_draw, dim3(ea_blocks(sh.added)), TILE, a, 0);
        if (a.one) {
            size_t sb = B.sort_bytes;
            RLAP_HIPCHK(rocprim::radix_sort_keys(B.sort_tmp, sb, (const uint64_t*)B.bin, B.bs, (size_t)sh.added, 0u, key_width(N) + view_bits(K), st));
            ++sorts;
        } else {
            for (int k = 0; k < K; ++k) {
                if (g.num_add[k] == 0) continue;
                size_t sb = B.sort_bytes;
                RLAP_HIPCHK(rocprim::radix_sort_keys(B.sort_tmp, sb, (const uint64_t*)B.bin + a.first[k], B.bs + a.first[k], (size_t)g.num_add[k], 0u,
                                                     key_width(N), st));
                ++sorts;
            }
        }
    }
    RLAP_LAUNCH_COUNTED(k_ea_heads_b, dim3(ea_blocks(sh.added + 1)), TILE, a);
    {
        size_t cb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.flag_b, B.pos_b, (int64_t)0, (size_t)(sh.added + 1), rocprim::plus<int64_t>(), st));
    }
    if (sh.added > 0) RLAP_LAUNCH_COUNTED(k_ea_runs_b, dim3(ea_blocks(sh.added)), TILE, a);
    // 3. list A and the merge
    Tail t{};
    t.w = g.w; t.E = E; t.words = B.words; t.flag_a = B.flag_a; t.pos_a = B.pos_a; t.akey = B.akey; t.asum = B.asum;
    t.bkey = B.bkey; t.bcnt = B.bcnt; t.pos_b = B.pos_b; t.K = K; t.b = a.b; t.nT = sh.nT; t.counts = B.counts; t.offs = B.offs;
    for (int k = 0; k <= K; ++k) t.first[k] = a.first[k];
    t.rows = g.rows; t.cap = g.cap; t.ptr = g.ptr; t.aptr = g.aptr;
    const int64_t slots = (int64_t)K * sh.nT + 1;
    auto tail = [&](const uint64_t* key, const int32_t* perm, int gate) -> int {
        t.key = key; t.perm = perm; t.gate = gate;
        RLAP_LAUNCH_COUNTED(k_ea_heads_a, dim3(ea_blocks(E + 1)), TILE, t);
        size_t cb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.flag_a, B.pos_a, (int64_t)0, (size_t)(E + 1), rocprim::plus<int64_t>(), st));
        RLAP_LAUNCH_COUNTED(k_ea_runs_a, dim3(ea_blocks(std::max<int64_t>(E, 1))), TILE, t);
        RLAP_HIPCHK(hipMemsetAsync(B.counts, 0, sizeof(int32_t) * (size_t)slots, st));
        RLAP_LAUNCH_COUNTED(k_ea_merge<false>, dim3((unsigned)sh.nT, (unsigned)K), TILE, t);
        cb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.counts, B.offs, (int64_t)0, (size_t)slots, rocprim::plus<int64_t>(), st));
        RLAP_LAUNCH_COUNTED(k_ea_ptr, dim3(1), WAVE, t);
        RLAP_LAUNCH_COUNTED(k_ea_merge<true>, dim3((unsigned)sh.nT, (unsigned)K), TILE, t);
        return RLAP_OK;
    };
    // for keys that ascend: the whole call; every kernel of it returns on the raised word
    if (const int rc = tail(B.kin, nullptr, 1)) return rc;
    // for keys that do not: the row total and ptr from a set of the input's keys; every kernel of it returns unless the word is raised
    if (E > 0) {
        RLAP_LAUNCH_COUNTED(k_ea_hash_clear, dim3(ea_blocks(a.slots)), TILE, a);
        RLAP_LAUNCH_COUNTED(k_ea_hash_insert, dim3(ea_blocks(E)), TILE, a);
        if (sh.added > 0) RLAP_LAUNCH_COUNTED(k_ea_hash_probe, dim3(ea_blocks(sh.max_add)), TILE, a);
        RLAP_LAUNCH_COUNTED(k_ea_hash_ptr, dim3(1), WAVE, a);
    }
    // the one read-back: the error word, whether the keys ascended, the distinct input keys and the row total
    RLAP_HIPCHK(hipMemcpyAsync(hw, B.words, sizeof(hw), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs = 1;
    const bool unsorted = !h32[W_ERR] && h32[W_UNSORTED];
    const bool fits = hw[W_TOTAL64] >= 0 && hw[W_TOTAL64] <= g.cap;
    if (unsorted && fits) {
        // the rows themselves need the sort; they follow in stream order, and nothing more is read back
        // (without weights every row weighs 1.0 and a run's sum is its length: the row numbers need not travel with the keys)
        size_t sb = B.sort_bytes;
        if (g.w) RLAP_HIPCHK(rocprim::radix_sort_pairs(B.sort_tmp, sb, (const uint64_t*)B.kin, B.ks, (const int32_t*)B.vin, B.perm, (size_t)E, 0u, key_width(N), st));
        else RLAP_HIPCHK(rocprim::radix_sort_keys(B.sort_tmp, sb, (const uint64_t*)B.kin, B.ks, (size_t)E, 0u, key_width(N), st));
        ++sorts;
        if (const int rc = tail(B.ks, g.w ? B.perm : nullptr, 0)) return rc;
    }
    rep->launches = launches;
    rep->sorts = sorts;
    rep->input_sorted = h32[W_UNSORTED] ? 0 : 1;
    if (h32[W_ERR]) return RLAP_E_INDEX_RANGE;
    rep->rows_needed = hw[W_TOTAL64];
    rep->input_distinct = hw[W_NA64];
    if (hw[W_TOTAL64] < 0 || hw[W_TOTAL64] > (int64_t)K * E + sh.added) return RLAP_E_INTERNAL;
    if (hw[W_TOTAL64] > g.cap) return RLAP_E_OUT_CAPACITY;
    return RLAP_OK;
}

}  // namespace rlap
