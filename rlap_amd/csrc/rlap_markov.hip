// rlap_markov.hip -- Markov diffusion of snapshots (rlap_snapshot_markov): for every segment s of a Schur-complement
// result (or a plain edge list), with Â = D^-1/2 A D^-1/2 on the segment's ids, beta = 1 - alpha and order D,
//     M = alpha Â + (1/D) sum_{k=0..D} beta^k Â^(k+1),  entries >= eps kept,  then (normalize_out) D_M^-1/2 M D_M^-1/2
// as sparse rows [i, j, value], row-major per segment -- without an n_s x n_s buffer anywhere.
//
// The prologue (column pass, weights, degrees, coefficients, ranks), the tile area and its table, and the epilogue (keep, sort, row
// sums, output) are those of the PPR diffusion (rlap_ppr_common.h).  A tile is (segment, 64 source blocks), two n_s x 64
// float64 copies with one row per node and one lane per source, run through the D + 1 applications of Â of rlap_markov.h (Horner
// form; every scalar step is a function of that header).  One wave per node computes sum_r a_r X[rb[r], lane] over the rows of its
// block in row order: a wave-uniform (a_r, rb[r]) and one 512-byte row gather per row, four in flight.  Two regimes, the same
// arithmetic in the same order in both:
//   small  segments up to PPR_SMALL_MAX nodes: one workgroup per tile runs all sweeps behind workgroup barriers
//   large  the others: one device-wide launch per sweep over a group's rows, wave = row
// (A third regime with both copies of a tile in LDS for segments up to 128 nodes was built and measured; on a batch of 128 small
// graphs it was not faster than the small regime by more than the run-to-run spread, so it was left out: DESIGN 4.23.)
// After the last sweep every tile keeps its entries with rank(row id) >= rank(source id) and value >= eps, as in 4.8: the result is
// exactly symmetric, no atomics touch a floating-point value, and a segment's arithmetic does not depend on the other segments.
#include "rlap_markov_api.h"
#include "rlap_ppr_common.h"   // the prologue, the tile area, the epilogue (shared with rlap_ppr.hip)

namespace rlap {
namespace {

// (Â x) at node row i of a tile (segment blocks from b0) for this lane's source: the rows of the block in row order, then the
// diagonal term.  i is wave-uniform.
__device__ inline double mk_apply(const Tiles& T, int64_t b0, int64_t i, const double* __restrict__ cur, int lane) {
    const int32_t r0 = T.bstart[b0 + i], r1 = T.bstart[b0 + i + 1];
    double acc = 0.0;
    int32_t r = r0;
    for (; r + 4 <= r1; r += 4) {   // (four gathers in flight, summed in row order)
        const double x0 = cur[(int64_t)(T.rb[r] - b0) * PPR_TILE + lane];
        const double x1 = cur[(int64_t)(T.rb[r + 1] - b0) * PPR_TILE + lane];
        const double x2 = cur[(int64_t)(T.rb[r + 2] - b0) * PPR_TILE + lane];
        const double x3 = cur[(int64_t)(T.rb[r + 3] - b0) * PPR_TILE + lane];
        acc += T.a[r] * x0;
        acc += T.a[r + 1] * x1;
        acc += T.a[r + 2] * x2;
        acc += T.a[r + 3] * x3;
    }
    for (; r < r1; ++r) acc += T.a[r] * cur[(int64_t)(T.rb[r] - b0) * PPR_TILE + lane];
    acc += T.cdiag[b0 + i] * cur[i * PPR_TILE + lane];
    return acc;
}

// application m (0 .. D) at node row i: reads cur, writes nxt (rlap_markov.h: m < D a Horner step, the last of them on to u; m = D
// the entry of M)
__device__ inline void mk_row_step(const Tiles& T, int64_t b0, int64_t c0, int64_t i, int32_t m, const double* __restrict__ cur,
                                   double* __restrict__ nxt, int lane) {
    const double acc = mk_apply(T, b0, i, cur, lane);
    const bool src = c0 + lane == i;
    nxt[i * PPR_TILE + lane] = m < T.K ? markov::step(acc, src, T.alpha, markov::beta_of(T.alpha), T.K, m) : markov::last(acc);
}

// h_0 = e_j in the first copy of every tile of a group (the second is written by application 0 before it is read)
__global__ void k_mk_init(Tiles T, const int64_t* __restrict__ gt, int64_t nt) {
    const int64_t t = gt[0] + blockIdx.y;
    if (blockIdx.y >= nt) return;
    const int64_t* d = T.tab + t * T_FIELDS;
    const int64_t s = d[T_SEG], c0 = d[T_C0];
    const int64_t n = T.sb[s + 1] - T.sb[s];
    double* x0 = T.x + d[T_XOFF];
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * PPR_TILE; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / PPR_TILE, l = e % PPR_TILE;
        x0[e] = c0 + l == i ? 1.0 : 0.0;
    }
}

// small regime: one workgroup runs all D + 1 applications of one tile
__global__ __launch_bounds__(PP_SMALL_THREADS) void k_mk_small(Tiles T, const int64_t* __restrict__ gt) {
    const int64_t t = gt[0] + blockIdx.x;
    const int64_t* d = T.tab + t * T_FIELDS;
    const int64_t s = d[T_SEG], c0 = d[T_C0];
    const int64_t b0 = T.sb[s], n = T.sb[s + 1] - b0;
    double* xa = T.x + d[T_XOFF];
    double* xb = xa + n * PPR_TILE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int32_t m = 0; m <= T.K; ++m) {
        const double* cur = (m & 1) ? xb : xa;
        double* nxt = (m & 1) ? xa : xb;
        for (int64_t i = wave; i < n; i += PP_SMALL_THREADS / 64) mk_row_step(T, b0, c0, i, m, cur, nxt, lane);
        __syncthreads();
    }
}

// large regime, application m over the rows of a group: wave q of the launch is row q of the group (tiles in order, T_ROFF ascending)
__global__ __launch_bounds__(PP_THREADS) void k_mk_large(Tiles T, const int64_t* __restrict__ gt, int64_t nt, int64_t rows, int32_t m) {
    const int64_t q = (int64_t)blockIdx.x * (PP_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= rows) return;
    int64_t lo = 0, hi = nt;   // tile of row q: the last u with roff[u] <= q
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (T.tab[(gt[0] + mid) * T_FIELDS + T_ROFF] <= q) lo = mid; else hi = mid;
    }
    const int64_t* d = T.tab + (gt[0] + lo) * T_FIELDS;
    const int64_t s = d[T_SEG], c0 = d[T_C0];
    const int64_t b0 = T.sb[s], n = T.sb[s + 1] - b0;
    double* xa = T.x + d[T_XOFF];
    double* xb = xa + n * PPR_TILE;
    const int lane = threadIdx.x & 63;
    const double* cur = (m & 1) ? xb : xa;
    double* nxt = (m & 1) ? xa : xb;
    mk_row_step(T, b0, c0, q - d[T_ROFF], m, cur, nxt, lane);
}

}  // namespace

size_t snapshot_markov_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int64_t out_cap) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_ppr(C, m, S, G, N, out_cap, 1, B);
}

int snapshot_markov_run(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotMarkovArgs& a, SnapshotMarkovReport* rep) {
    *rep = SnapshotMarkovReport{};
    const SnapshotSeg& in = a.seg;
    const int weighted = (a.flags & RLAP_MARKOV_WEIGHTED) ? 1 : 0, self_loop = (a.flags & RLAP_MARKOV_SELF_LOOP) ? 1 : 0;
    const int normalize = (a.flags & RLAP_MARKOV_NORMALIZE) ? 1 : 0, zero_ok = (a.flags & RLAP_MARKOV_ZERO_ROWS) ? 1 : 0;
    // 1. to 3. the tables, the column pass, the weights, degrees, coefficients w / sqrt(d d') and ranks (rlap_ppr_common.h)
    Prologue P;
    int rc = pp_prologue(st, ws, ws_bytes, in, a.out_cap, 1, weighted, self_loop, zero_ok, 0, 1.0, a.out_ptr, &P);
    rep->host_syncs = P.host_syncs;
    if (rc != RLAP_OK || P.done) return rc;
    const Bufs& B = P.B;
    // 4. tiles and groups (rlap_ppr_tiles.h: small segments' tiles first)
    pprtiles::Table tt;
    pprtiles::build(P.hnodes.data(), in.S, &tt);
    rep->small_tiles = tt.small_tiles;
    rep->large_tiles = tt.large_tiles;
    const int64_t ntiles = tt.ntiles();
    const int64_t ngroups = tt.ngroups();
    rc = pp_upload_table(st, tt, P);
    if (rc != RLAP_OK) return rc;
    rep->groups = ngroups;
    Tiles T{B.tab, nullptr, in.sc, B.col.bstart, B.col.rb, B.col.sb, B.a, B.cdiag, B.rank, B.x, a.alpha, a.eps, a.order,
            markov::final_copy(a.order)};
    // 5. the sweeps, group by group; after application D each group's kept entries are counted, scanned and staged
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t* gt = B.gt + g;
        const int64_t nt = (g + 1 < ngroups ? tt.gstart[(size_t)g + 1] : ntiles) - tt.gstart[(size_t)g];
        const int64_t rows = tt.grows[(size_t)g];
        hipLaunchKernelGGL(k_mk_init, dim3(64, (unsigned)nt), dim3(PP_THREADS), 0, st, T, gt, nt);
        rep->launches += 1;
        if (tt.gsmall[(size_t)g]) {
            hipLaunchKernelGGL(k_mk_small, dim3((unsigned)nt), dim3(PP_SMALL_THREADS), 0, st, T, gt);
            rep->launches += 1;
        } else {
            for (int32_t m = 0; m <= a.order; ++m) {
                hipLaunchKernelGGL(k_mk_large, dim3(grid_blocks(rows, PP_THREADS / 64)), dim3(PP_THREADS), 0, st, T, gt, nt, rows, m);
                rep->launches += 1;
            }
        }
        RLAP_HIPCHK(hipGetLastError());
        rc = pp_group_keep(st, T, B, gt, nt, rows, a.out_cap);
        if (rc != RLAP_OK) return rc;
        rep->launches += 4;
    }
    // 6. and 7. the kept count, read back once; (segment, i, j) order, row sums, the output rows and offsets (rlap_ppr_common.h)
    rc = pp_epilogue(st, in, &P, normalize, a.out, a.out_cap, a.out_ptr, &rep->kept);
    rep->host_syncs = P.host_syncs;
    return rc;
}

}  // namespace rlap
