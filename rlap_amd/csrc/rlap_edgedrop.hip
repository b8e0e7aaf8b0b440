// rlap_edgedrop.hip -- centrality-adaptive edge dropping, K views a call (rlap_edge_drop).  The rules -- counts,
// centralities, scores, drop probability, coin and the order of every sum -- are rlap_edgedrop.h's.  A translation unit of its own.
//
//   keys     one pass over the rows: both ids checked (a row that fails raises the error word; every later kernel returns on a raised
//            word), in[] / out[] counted (integer atomics, one per run of equal ids in a wave), the target key and the row number for the sort, or (degree) the two
//            64-bit keys v * N + u of the row.
//   lists    pagerank / eigenvector: rocPRIM's stable radix sort of (target, row) gives every node's incoming rows in input order;
//            their 4-byte source ids are stored in list order.  degree: one sort of the 2E pair keys, the heads counted per v.
//   steps    one launch a step of an iteration; kernel boundaries carry the data between workgroups.  Every kernel of an eigenvector
//            step returns at once when the `done` word is set: the host enqueues max_iter steps and reads nothing back.
//   scores   three node-level kernels over tiles of 256 nodes with partials.
//   flip     the only per-edge kernels, rlap_rowcompact_dev.h's two passes (k_rc_count, k_rc_ptr, k_rc_write) with the predicate
//            DropCoin: the coin of (view, row) against the drop probability, recomputed in pass B, which also writes the optional
//            mask.
//   One read-back: the error word, the iteration report and the row total.  No atomic on a float; LDS holds reduction words only.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_edgedrop.h"
#include "rlap_rowcompact_dev.h"
#include "rlap_snapshot.h"

namespace rlap {
namespace {

using namespace edgedrop;
using rowcompact::clamp;

constexpr int64_t ED_MAX_GRID = 8192;                    // workgroups of a strided launch
enum { W_ERR = 0, W_DONE = 1, W_ITERS = 2, W_CONV = 3, W_TOTAL64 = 2, W_WORDS64 = 4 };   // int32 words; the total is int64 word 2

inline unsigned ed_blocks(int64_t n) { return capped_blocks(n, TILE, ED_MAX_GRID); }

struct Ed {
    const int64_t* src; const int64_t* dst; int64_t E, N, nt;   // nt: node tiles
    int scheme, source;
    int32_t* words;
    int32_t* in; int32_t* out;
    uint32_t* key; int32_t* val; int32_t* lo; int32_t* hi; int32_t* srcs;
    uint64_t* key2; uint64_t* skey2; int32_t* dcount;
    double* c; double* s; double* wv; double* nw; double* x; double* y; double* part;   // part: [3][nt]
};

__device__ inline bool ed_failed(const Ed& a) { return a.words[W_ERR] != 0; }
__device__ inline const int32_t* ed_cnt(const Ed& a) { return a.source ? a.out : a.in; }

template <class Op>
__device__ inline double wg_reduce(Op op, double v, double* red) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
    __syncthreads();   // (red may still be read by the previous call)
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = v;
    __syncthreads();
    return combine_waves(op, red[0], red[1], red[2], red[3]);
}

template <class Op>
__device__ inline double wg_total(Op op, const double* __restrict__ part, int64_t n, double* red) {
    double p = op.identity();
    for (int64_t t = threadIdx.x; t < n; t += TILE) p = op(p, part[t]);
    return wg_reduce(op, p, red);
}

// the list of node v (lanes past the last node: n = 0), 16 lanes wide: every lane of the group returns the sum
__device__ inline double ed_list_sum(const Ed& a, int64_t v, int sub, const double* __restrict__ x) {
    int64_t s = 0, n = 0;
    if (v < a.N) {
        s = clamp(a.lo[v], 0, a.E);
        n = clamp(a.hi[v], s, a.E) - s;
    }
    double acc[edgeplan::ACCS] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t turn = 0; edgeplan::place_of(turn, 0, sub) < n; ++turn) {
#pragma unroll
        for (int u = 0; u < edgeplan::ACCS; ++u) {
            const int64_t k = edgeplan::place_of(turn, u, sub);
            if (k < n) acc[u] += x[clamp(a.srcs[s + k], 0, a.N - 1)];
        }
    }
    double d = edgeplan::combine(acc);
#pragma unroll
    for (int o = edgeplan::LANES / 2; o > 0; o >>= 1) d = edgeplan::meet(d, __shfl_xor(d, o));
    return d;
}

// arr[idx] += the lanes of a run that count: a run is neighbouring live lanes of a wave with the same idx (rows sorted by an id come
// in runs), and its first lane makes the one atomic (integer adds, so the order does not matter).  Every lane of the wave calls it.
__device__ inline void run_add(int32_t* __restrict__ arr, int64_t idx, bool live, bool counts) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t prev = __shfl_up(idx, 1);
    const unsigned long long lv = __ballot(live), cn = __ballot(live && counts);
    const bool lead = live && (lane == 0 || !(lv >> (lane - 1) & 1ull) || prev != idx);
    const unsigned long long leads = __ballot(lead);
    if (!lead) return;
    const unsigned long long above = lane == WAVE - 1 ? 0ull : ~0ull << (lane + 1);
    const unsigned long long stop = (leads | ~lv) & above;   // the next run's first lane, or the next lane that is not live
    const int end = stop ? __ffsll(stop) - 1 : WAVE;
    const unsigned long long span = (end == WAVE ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
    const int n = __popcll(cn & span);
    if (n) atomicAdd(&arr[idx], n);
}

__global__ __launch_bounds__(TILE) void k_ed_keys(Ed a, int counts, int csr, int pairs) {
    const int64_t stride = (int64_t)gridDim.x * TILE, rounds = (a.E + stride - 1) / stride;   // (whole waves stay in the loop)
    int64_t e = (int64_t)blockIdx.x * TILE + threadIdx.x;
    for (int64_t r = 0; r < rounds; ++r, e += stride) {
        const bool live = e < a.E;
        const int64_t s = live ? a.src[e] : 0, d = live ? a.dst[e] : 0;
        const bool ok = live && s >= 0 && s < a.N && d >= 0 && d < a.N;
        if (live && !ok) atomicOr(&a.words[W_ERR], 1);
        if (counts) { run_add(a.in, d, ok, true); run_add(a.out, s, ok, true); }
        if (!live) continue;
        if (csr) { a.key[e] = ok ? (uint32_t)d : 0u; a.val[e] = (int32_t)e; }
        if (pairs) {
            a.key2[2 * e] = ok ? (uint64_t)d * (uint64_t)a.N + (uint64_t)s : 0ull;
            a.key2[2 * e + 1] = ok ? (uint64_t)s * (uint64_t)a.N + (uint64_t)d : 0ull;
        }
    }
}

// degree: the heads of the sorted pair keys, counted per v
__global__ __launch_bounds__(TILE) void k_ed_heads(Ed a) {
    if (ed_failed(a)) return;
    const int64_t stride = (int64_t)gridDim.x * TILE, rounds = (2 * a.E + stride - 1) / stride;   // (whole waves stay in the loop)
    int64_t p = (int64_t)blockIdx.x * TILE + threadIdx.x;
    for (int64_t r = 0; r < rounds; ++r, p += stride) {
        bool head = false;
        uint64_t v = 0;
        if (p < 2 * a.E) {
            const uint64_t key = a.skey2[p];
            head = p == 0 || a.skey2[p - 1] != key;
            v = key / (uint64_t)a.N;
        }
        run_add(a.dcount, (int64_t)v, p < 2 * a.E && v < (uint64_t)a.N, head);
    }
}

__global__ __launch_bounds__(TILE) void k_ed_degree(Ed a) {
    if (ed_failed(a)) return;
    for (int64_t v = (int64_t)blockIdx.x * TILE + threadIdx.x; v < a.N; v += (int64_t)gridDim.x * TILE) a.c[v] = (double)a.dcount[v];
}

__global__ __launch_bounds__(TILE) void k_ed_fill(double* __restrict__ x, int64_t n, double value) {
    for (int64_t v = (int64_t)blockIdx.x * TILE + threadIdx.x; v < n; v += (int64_t)gridDim.x * TILE) x[v] = value;
}

// a PageRank step, part 1: z[u] = x[u] / out[u], so that the gather is 8 bytes an edge
__global__ __launch_bounds__(TILE) void k_ed_pr_share(Ed a, const double* __restrict__ x, double* __restrict__ z) {
    if (ed_failed(a)) return;
    for (int64_t v = (int64_t)blockIdx.x * TILE + threadIdx.x; v < a.N; v += (int64_t)gridDim.x * TILE) z[v] = pr_share(x[v], a.out[v]);
}

// part 2: x[v] = (1 - damp) x[v] + damp * list_v(z), 16 lanes a node
__global__ __launch_bounds__(TILE) void k_ed_pr_gather(Ed a, double* __restrict__ x, const double* __restrict__ z, double damp) {
    if (ed_failed(a)) return;
    const int sub = threadIdx.x & (edgeplan::LANES - 1);
    const int64_t stride = (int64_t)gridDim.x * TILE / edgeplan::LANES;
    const int64_t rounds = (a.N + stride - 1) / stride;   // (whole waves stay in the loop: the butterflies need their lanes)
    int64_t v = ((int64_t)blockIdx.x * TILE + threadIdx.x) / edgeplan::LANES;
    for (int64_t r = 0; r < rounds; ++r, v += stride) {
        const double sum = ed_list_sum(a, v, sub, z);
        if (sub == 0 && v < a.N) x[v] = pr_update(x[v], sum, damp);
    }
}

// an eigenvector step, part 1: y[v] = x[v] + list_v(x) for the tile's nodes, the tile's partial of y * y
__global__ __launch_bounds__(TILE) void k_ed_evc_gather(Ed a) {
    __shared__ double red[4];
    if (ed_failed(a) || a.words[W_DONE]) return;
    const int sub = threadIdx.x & (edgeplan::LANES - 1), grp = threadIdx.x / edgeplan::LANES;
    const int64_t v0 = (int64_t)blockIdx.x * TILE;
    for (int pass = 0; pass < edgeplan::LANES; ++pass) {
        const int64_t v = v0 + pass * (TILE / edgeplan::LANES) + grp;
        const double sum = ed_list_sum(a, v, sub, a.x);
        if (sub == 0 && v < a.N) a.y[v] = a.x[v] + sum;
    }
    __syncthreads();   // (the tile's y is this workgroup's own)
    const int64_t v = v0 + threadIdx.x;
    double t = 0.0;
    if (v < a.N) { const double y = a.y[v]; t = y * y; }
    const double r = wg_reduce(Add(), t, red);
    if (threadIdx.x == 0) a.part[blockIdx.x] = r;
}

// part 2: x' = y / ||y||, the tile's partial of |x' - x|
__global__ __launch_bounds__(TILE) void k_ed_evc_norm(Ed a) {
    __shared__ double red[4];
    if (ed_failed(a) || a.words[W_DONE]) return;
    const double nrm = sqrt(wg_total(Add(), a.part, a.nt, red));
    const int64_t v = (int64_t)blockIdx.x * TILE + threadIdx.x;
    double d = 0.0;
    if (v < a.N) {
        const double xn = a.y[v] / nrm;
        d = fabs(xn - a.x[v]);
        a.x[v] = xn;
    }
    const double r = wg_reduce(Add(), d, red);
    if (threadIdx.x == 0) a.part[a.nt + blockIdx.x] = r;
}

// part 3, one workgroup: the stopping decision
__global__ __launch_bounds__(TILE) void k_ed_evc_check(Ed a, double tol) {
    __shared__ double red[4];
    if (ed_failed(a) || a.words[W_DONE]) return;
    const double err = wg_total(Add(), a.part + a.nt, a.nt, red);   // (its barriers: every lane has read the words by now)
    if (threadIdx.x != 0) return;
    a.words[W_ITERS] += 1;
    if (evc_stops(err, a.N, tol)) { a.words[W_DONE] = 1; a.words[W_CONV] = 1; }
}

__global__ __launch_bounds__(TILE) void k_ed_evc_finish(Ed a) {
    if (ed_failed(a)) return;
    for (int64_t v = (int64_t)blockIdx.x * TILE + threadIdx.x; v < a.N; v += (int64_t)gridDim.x * TILE) a.c[v] = evc_finish(a.x[v]);
}

// scores, one tile of nodes a workgroup: s and the partials of smax and cnt * s
__global__ __launch_bounds__(TILE) void k_ed_score_s(Ed a) {
    __shared__ double red[4];
    if (ed_failed(a)) return;
    const int64_t v = (int64_t)blockIdx.x * TILE + threadIdx.x;
    double mx = Max().identity(), sm = 0.0;
    if (v < a.N) {
        const double s = log(a.c[v]);
        const int32_t cnt = ed_cnt(a)[v];
        a.s[v] = s;
        mx = max_term(cnt, s);
        sm = weighted_term(cnt, s);
    }
    const double rm = wg_reduce(Max(), mx, red);
    const double rs = wg_reduce(Add(), sm, red);
    if (threadIdx.x == 0) { a.part[blockIdx.x] = rm; a.part[a.nt + blockIdx.x] = rs; }
}

// w and the partial of cnt * w
__global__ __launch_bounds__(TILE) void k_ed_score_w(Ed a) {
    __shared__ double red[4];
    if (ed_failed(a)) return;
    const double smax = wg_total(Max(), a.part, a.nt, red);
    const double smean = wg_total(Add(), a.part + a.nt, a.nt, red) / (double)a.E;
    const int64_t v = (int64_t)blockIdx.x * TILE + threadIdx.x;
    double t = 0.0;
    if (v < a.N) {
        const double w = score_w(smax, smean, a.s[v]);
        a.wv[v] = w;
        t = weighted_term(ed_cnt(a)[v], w);
    }
    const double r = wg_reduce(Add(), t, red);
    if (threadIdx.x == 0) a.part[2 * a.nt + blockIdx.x] = r;
}

__global__ __launch_bounds__(TILE) void k_ed_score_nw(Ed a) {
    __shared__ double red[4];
    if (ed_failed(a)) return;
    const double wmean = wg_total(Add(), a.part + 2 * a.nt, a.nt, red) / (double)a.E;
    const int64_t v = (int64_t)blockIdx.x * TILE + threadIdx.x;
    if (v < a.N) a.nw[v] = a.wv[v] / wmean;
}

// ---------------------------------------------------------------- flip and compact: rlap_rowcompact_dev.h's passes with this predicate
struct DropCoin {
    static constexpr bool MASK = true;
    struct Row { uint64_t he; double nw; };   // the hash of the row number and the node weight of the endpoint
    int uniform, source; int64_t N;
    const double* nw; double p[MAX_VIEWS]; double threshold; uint64_t seed;
    __device__ Row row(const rowcompact::Rows& c, int64_t e) const {
        Row r{coin_row(e), 0.0};
        if (!uniform && e < c.E) r.nw = nw[clamp(source ? c.src[e] : c.dst[e], 0, N - 1)];
        return r;
    }
    __device__ uint64_t view(int k) const { return coin_view(seed, k); }
    __device__ bool keep(int k, uint64_t view, const Row& r) const {
        return keeps(coin_of(view, r.he), drop_prob(uniform != 0, r.nw, p[k], threshold));
    }
};

struct Bufs {
    int32_t* words;
    int32_t *in, *out, *val, *perm, *lo, *hi, *srcs, *dcount;
    uint32_t *key, *skey;
    uint64_t *key2, *skey2;
    double *c, *s, *wv, *nw, *x, *y, *part;
    rowcompact::Scratch compact;
    void* sort_tmp; size_t sort_bytes;
};

size_t carve(Carve& C, int64_t E, int64_t N, int K, int scheme, Bufs& B) {
    const bool scored = scheme != UNIFORM, csr = scheme == PAGERANK || scheme == EIGENVECTOR, pairs = scheme == DEGREE;
    const int64_t nt = tiles(N), nT = row_tiles(E);
    B.words = C.take<int32_t>(2 * W_WORDS64);
    B.in = C.take<int32_t>(scored ? N : 0);
    B.out = C.take<int32_t>(scored ? N : 0);
    B.key = C.take<uint32_t>(csr ? E : 0);
    B.skey = C.take<uint32_t>(csr ? E : 0);
    B.val = C.take<int32_t>(csr ? E : 0);
    B.perm = C.take<int32_t>(csr ? E : 0);
    B.srcs = C.take<int32_t>(csr ? E : 0);
    B.lo = C.take<int32_t>(csr ? N : 0);
    B.hi = C.take<int32_t>(csr ? N : 0);
    B.key2 = C.take<uint64_t>(pairs ? 2 * E : 0);
    B.skey2 = C.take<uint64_t>(pairs ? 2 * E : 0);
    B.dcount = C.take<int32_t>(pairs ? N : 0);
    B.c = C.take<double>(scored ? N : 0);
    B.s = C.take<double>(scored ? N : 0);
    B.wv = C.take<double>(scored ? N : 0);
    B.nw = C.take<double>(scored ? N : 0);
    B.x = C.take<double>(csr ? N : 0);
    B.y = C.take<double>(csr ? N : 0);
    B.part = C.take<double>(scored ? 3 * nt : 0);
    rowcompact::carve(C, K, nT, B.compact);
    B.sort_bytes = csr ? rowcompact::list_sort_bytes(E, N) : 0;
    if (pairs)
        (void)rocprim::radix_sort_keys(nullptr, B.sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)std::max<int64_t>(2 * E, 1), 0u,
                                       pair_key_bits(N), (hipStream_t)0);
    B.sort_tmp = C.take<char>((int64_t)B.sort_bytes);
    return C.off + 256;
}

}  // namespace

size_t edge_drop_bytes(int64_t E, int64_t N, int K, int scheme) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve(C, E, N, K, scheme, B);
}

int edge_drop_run(hipStream_t st, void* ws, size_t ws_bytes, const EdgeDropArgs& g, EdgeDropReport* rep) {
    *rep = EdgeDropReport{};
    const int64_t E = g.E, N = g.N, nt = tiles(N), nT = row_tiles(E);
    const int K = g.K, scheme = g.scheme;
    const bool scored = scheme != UNIFORM && E > 0 && N > 0, csr = scored && (scheme == PAGERANK || scheme == EIGENVECTOR), pairs = scored && scheme == DEGREE;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve(C, E, N, K, scheme, B) > ws_bytes) return RLAP_E_WORKSPACE;
    int64_t launches = 0;
    Ed a{};
    a.src = g.src; a.dst = g.dst; a.E = E; a.N = N; a.nt = nt; a.scheme = scheme; a.source = g.source;
    a.words = B.words; a.in = B.in; a.out = B.out;
    a.key = B.key; a.val = B.val; a.lo = B.lo; a.hi = B.hi; a.srcs = B.srcs;
    a.key2 = B.key2; a.skey2 = B.skey2; a.dcount = B.dcount;
    a.c = g.centrality ? g.centrality : B.c; a.s = B.s; a.wv = B.wv; a.nw = g.node_weight ? g.node_weight : B.nw;
    a.x = B.x; a.y = B.y; a.part = B.part;
    RLAP_HIPCHK(hipMemsetAsync(B.words, 0, sizeof(int64_t) * W_WORDS64, st));
    if (!scored && N > 0) {   // (uniform, or no rows: nothing to score)
        if (g.centrality) RLAP_HIPCHK(hipMemsetAsync(g.centrality, 0, sizeof(double) * (size_t)N, st));
        if (g.node_weight) RLAP_HIPCHK(hipMemsetAsync(g.node_weight, 0, sizeof(double) * (size_t)N, st));
    }
    // 1. keys and counts, the lists
    if (scored) {
        RLAP_HIPCHK(hipMemsetAsync(B.in, 0, sizeof(int32_t) * (size_t)N, st));
        RLAP_HIPCHK(hipMemsetAsync(B.out, 0, sizeof(int32_t) * (size_t)N, st));
    }
    if (E > 0) RLAP_LAUNCH_COUNTED(k_ed_keys, ed_blocks(E), TILE, a, scored ? 1 : 0, csr ? 1 : 0, pairs ? 1 : 0);
    if (csr) {
        // every node's incoming rows in input order, their sources in list order
        const rowcompact::Lists l{E, N, B.words + W_ERR, B.key, B.val, B.skey, B.perm, B.lo, B.hi, g.src, B.srcs, B.sort_tmp, B.sort_bytes};
        if (const int rc = rowcompact::build_lists(st, l, ed_blocks(E), launches)) return rc;
    }
    // 2. the centrality
    if (pairs) {
        RLAP_HIPCHK(hipMemsetAsync(B.dcount, 0, sizeof(int32_t) * (size_t)N, st));
        size_t sb = B.sort_bytes;
        RLAP_HIPCHK(rocprim::radix_sort_keys(B.sort_tmp, sb, (const uint64_t*)B.key2, B.skey2, (size_t)(2 * E), 0u, pair_key_bits(N), st));
        RLAP_LAUNCH_COUNTED(k_ed_heads, ed_blocks(2 * E), TILE, a);
        RLAP_LAUNCH_COUNTED(k_ed_degree, ed_blocks(N), TILE, a);
    }
    if (csr && scheme == PAGERANK) {
        double* x = a.c;   // (the iterate is the centrality)
        RLAP_LAUNCH_COUNTED(k_ed_fill, ed_blocks(N), TILE, x, N, 1.0);
        for (int64_t it = 0; it < g.pr_iters; ++it) {
            RLAP_LAUNCH_COUNTED(k_ed_pr_share, ed_blocks(N), TILE, a, (const double*)x, B.y);
            RLAP_LAUNCH_COUNTED(k_ed_pr_gather, ed_blocks(N * edgeplan::LANES), TILE, a, x, (const double*)B.y, g.damp);
        }
    }
    if (csr && scheme == EIGENVECTOR) {
        RLAP_LAUNCH_COUNTED(k_ed_fill, ed_blocks(N), TILE, B.x, N, evc_start(N));
        for (int64_t it = 0; it < g.evc_max_iter; ++it) {
            RLAP_LAUNCH_COUNTED(k_ed_evc_gather, (unsigned)nt, TILE, a);
            RLAP_LAUNCH_COUNTED(k_ed_evc_norm, (unsigned)nt, TILE, a);
            RLAP_LAUNCH_COUNTED(k_ed_evc_check, 1, TILE, a, g.evc_tol);
        }
        RLAP_LAUNCH_COUNTED(k_ed_evc_finish, ed_blocks(N), TILE, a);
    }
    // 3. the scores
    if (scored) {
        RLAP_LAUNCH_COUNTED(k_ed_score_s, (unsigned)nt, TILE, a);
        RLAP_LAUNCH_COUNTED(k_ed_score_w, (unsigned)nt, TILE, a);
        RLAP_LAUNCH_COUNTED(k_ed_score_nw, (unsigned)nt, TILE, a);
    }
    // 4. flip and compact
    DropCoin p{};
    p.uniform = scheme == UNIFORM ? 1 : 0; p.source = g.source; p.N = N; p.nw = a.nw;
    for (int k = 0; k < K; ++k) p.p[k] = g.p[k];
    p.threshold = g.threshold; p.seed = g.seed;
    const rowcompact::Rows c{g.src, g.dst, g.w, E, nT, K, B.words + W_ERR, B.compact.counts, B.compact.offs, g.rows, g.cap, g.ptr, g.mask,
                             reinterpret_cast<int64_t*>(B.words) + W_TOTAL64};
    if (const int rc = rowcompact::run(st, c, p, B.compact, nT > 0, launches)) return rc;
    // 5. the error word, the iteration report and the total, read back once
    int64_t hw[W_WORDS64];
    RLAP_HIPCHK(hipMemcpyAsync(hw, B.words, sizeof(hw), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    const int32_t* h32 = reinterpret_cast<const int32_t*>(hw);
    rep->host_syncs = 1;
    rep->launches = launches;
    rep->iters = csr && scheme == EIGENVECTOR ? h32[W_ITERS] : (scheme == PAGERANK ? (int32_t)g.pr_iters : 0);   // (as the mirror: no rows, the same report)
    rep->converged = csr && scheme == EIGENVECTOR ? h32[W_CONV] : 1;
    if (h32[W_ERR]) return RLAP_E_INDEX_RANGE;
    rep->rows_needed = hw[W_TOTAL64];
    if (hw[W_TOTAL64] < 0 || hw[W_TOTAL64] > (int64_t)K * E) return RLAP_E_INTERNAL;
    if (hw[W_TOTAL64] > g.cap) return RLAP_E_OUT_CAPACITY;
    return RLAP_OK;
}

}  // namespace rlap
