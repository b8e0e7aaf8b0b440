// rlap_ppr.hip -- PPR diffusion of snapshots (rlap_snapshot_ppr): for every segment s of a Schur-complement result,
//     S = alpha (I - (1 - alpha) D^-1/2 A D^-1/2)^-1 on the segment's ids, entries >= eps kept, then (normalize_out) D_S^-1/2 S D_S^-1/2
// as sparse rows [i, j, value], row-major per segment -- without an n_s x n_s buffer anywhere.
//
// The column pass (rlap_snapshot.hip) numbers the segment's blocks (one per column id) and maps every row to the block of its row id.
// Columns of S are found 64 at a time: a tile is (segment, 64 source blocks), an n_s x 64 float64 matrix with one row per node and
// one lane per source, run through the K fixed Chebyshev steps of rlap_cheb.h (two live copies for the three-term recurrence; the
// new iterate overwrites x_{k-1} in place).  One wave per node computes sum_r a_r X[rb[r], lane] over the rows of its block in row
// order: a wave-uniform (a_r, rb[r]) and one 512-byte row gather per row.  Tiles of segments up to PPR_SMALL_MAX nodes run their K
// steps in one workgroup each; larger segments step together, one device-wide launch per step over a group of tiles.  Groups keep
// the live tile bytes within PPR_TILE_BUDGET (or one tile, when a single tile is larger).
//
// After step K every tile keeps its entries with rank(row id) >= rank(source id) and value >= eps: the pair {i, j} takes its value
// from the column of the smaller id, and both directions are staged with it (key (position of i, rank of j), value).  One radix sort
// puts them in (segment, i, j) order; row sums run over each sorted row in a fixed order, and the output pass normalises with
// v * (D_i^-1/2 D_j^-1/2) -- exactly symmetric.  No atomics touch a floating-point value, so a call gives the same bits every time,
// and a segment's arithmetic does not depend on the other segments of the call.
#include "rlap_cheb.h"
#include "rlap_ppr.h"
#include "rlap_ppr_common.h"   // the prologue, the tile area, the epilogue (shared with rlap_markov.hip)

namespace rlap {
namespace {

// one step of one node row i of a tile (segment blocks from b0, sources from c0): x_{k+1} = om (B x_k + f - x_{k-1}) + x_{k-1},
// written over x_{k-1}.  i is wave-uniform.
__device__ inline void tile_row_step(const Tiles& T, int64_t b0, int64_t c0, int64_t i, double om, const double* __restrict__ cur,
                                     double* __restrict__ prv, int lane) {
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
    const int64_t e = i * PPR_TILE + lane;
    acc += T.cdiag[b0 + i] * cur[e];
    if (c0 + lane == i) acc += T.alpha;
    prv[e] = cheb::step(om, acc, prv[e]);
}

// x_1 = f (alpha at (source row, source lane); zero when K = 0) and x_0 = 0 for every tile of a group
__global__ void k_pp_init(Tiles T, const int64_t* __restrict__ gt, int64_t nt) {
    const int64_t t = gt[0] + blockIdx.y;
    if (blockIdx.y >= nt) return;
    const int64_t* d = T.tab + t * T_FIELDS;
    const int64_t s = d[T_SEG], c0 = d[T_C0];
    const int64_t n = T.sb[s + 1] - T.sb[s];
    double* x0 = T.x + d[T_XOFF];
    double* x1 = x0 + n * PPR_TILE;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n * PPR_TILE; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / PPR_TILE, l = e % PPR_TILE;
        x0[e] = (T.K > 0 && c0 + l == i) ? T.alpha : 0.0;
        x1[e] = 0.0;
    }
}

// small regime: one workgroup runs all steps of one tile
__global__ __launch_bounds__(PP_SMALL_THREADS) void k_pp_small(Tiles T, const int64_t* __restrict__ gt) {
    const int64_t t = gt[0] + blockIdx.x;
    const int64_t* d = T.tab + t * T_FIELDS;
    const int64_t s = d[T_SEG], c0 = d[T_C0];
    const int64_t b0 = T.sb[s], n = T.sb[s + 1] - b0;
    double* xa = T.x + d[T_XOFF];
    double* xb = xa + n * PPR_TILE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int32_t k = 1; k < T.K; ++k) {
        const double* cur = (k & 1) ? xa : xb;
        double* prv = (k & 1) ? xb : xa;
        const double om = T.om[k];
        for (int64_t i = wave; i < n; i += PP_SMALL_THREADS / 64) tile_row_step(T, b0, c0, i, om, cur, prv, lane);
        __syncthreads();
    }
}

// large regime, step k over the rows of a group: wave q of the launch is row q of the group (tiles in order, T_ROFF ascending)
__global__ __launch_bounds__(PP_THREADS) void k_pp_large(Tiles T, const int64_t* __restrict__ gt, int64_t nt, int64_t rows, int32_t k) {
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
    const double* cur = (k & 1) ? xa : xb;
    double* prv = (k & 1) ? xb : xa;
    tile_row_step(T, b0, c0, q - d[T_ROFF], T.om[k], cur, prv, lane);
}

}  // namespace

size_t snapshot_ppr_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int64_t out_cap, int32_t K) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_ppr(C, m, S, G, N, out_cap, K, B);
}

int snapshot_ppr_run(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotPprArgs& a, SnapshotPprReport* rep) {
    *rep = SnapshotPprReport{};
    const SnapshotSeg& in = a.seg;
    const int weighted = (a.flags & RLAP_PPR_WEIGHTED) ? 1 : 0, self_loop = (a.flags & RLAP_PPR_SELF_LOOP) ? 1 : 0;
    const int normalize = (a.flags & RLAP_PPR_NORMALIZE) ? 1 : 0, zero_ok = (a.flags & RLAP_PPR_ZERO_ROWS) ? 1 : 0;
    // 1. to 3. the tables, the column pass, the weights, degrees, normalised weights (1 - alpha) w / sqrt(d d') and ranks
    // (rlap_ppr_common.h)
    Prologue P;
    int rc = pp_prologue(st, ws, ws_bytes, in, a.out_cap, a.K, weighted, self_loop, zero_ok, 1, 1.0 - a.alpha, a.out_ptr, &P);
    rep->host_syncs = P.host_syncs;
    if (rc != RLAP_OK || P.done) return rc;
    const Bufs& B = P.B;
    // 4. tiles and groups (rlap_ppr_tiles.h: small segments' tiles first), uploaded with the Chebyshev weights
    pprtiles::Table tt;
    pprtiles::build(P.hnodes.data(), in.S, &tt);
    rep->small_tiles = tt.small_tiles;
    rep->large_tiles = tt.large_tiles;
    const int64_t ntiles = tt.ntiles();
    const int64_t ngroups = tt.ngroups();
    rc = pp_upload_table(st, tt, P);
    if (rc != RLAP_OK) return rc;
    std::vector<double> om((size_t)std::max<int32_t>(a.K, 1));
    cheb::omegas(a.alpha, a.K, om.data());
    RLAP_HIPCHK(hipMemcpyAsync(B.om, om.data(), sizeof(double) * om.size(), hipMemcpyHostToDevice, st));
    rep->groups = ngroups;
    Tiles T{B.tab, B.om, in.sc, B.col.bstart, B.col.rb, B.col.sb, B.a, B.cdiag, B.rank, B.x, a.alpha, a.eps, a.K, (a.K & 1) ? 0 : 1};
    // 5. the sweeps, group by group; after step K (x_K lies in the first copy for an odd K; K = 0: the zero copy) each group's kept
    // entries are counted, scanned and staged
    for (int64_t g = 0; g < ngroups; ++g) {
        const int64_t* gt = B.gt + g;
        const int64_t nt = (g + 1 < ngroups ? tt.gstart[(size_t)g + 1] : ntiles) - tt.gstart[(size_t)g];
        const int64_t rows = tt.grows[(size_t)g];
        hipLaunchKernelGGL(k_pp_init, dim3(64, (unsigned)nt), dim3(PP_THREADS), 0, st, T, gt, nt);
        rep->launches += 1;
        if (tt.gsmall[(size_t)g]) {
            hipLaunchKernelGGL(k_pp_small, dim3((unsigned)nt), dim3(PP_SMALL_THREADS), 0, st, T, gt);
            rep->launches += 1;
        } else {
            for (int32_t k = 1; k < a.K; ++k) {
                hipLaunchKernelGGL(k_pp_large, dim3(grid_blocks(rows, PP_THREADS / 64)), dim3(PP_THREADS), 0, st, T, gt, nt, rows, k);
                rep->launches += 1;
            }
        }
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
