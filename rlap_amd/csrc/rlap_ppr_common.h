// rlap_ppr_common.h -- what the two diffusions of snapshots share (rlap_snapshot_ppr in rlap_ppr.hip, DESIGN 4.8, and
// rlap_snapshot_markov in rlap_markov.hip): the prologue (column pass, weight check, degrees, the coefficient of every
// row, ranks by id), the tile area and its table on the device, and the epilogue (keep count / scan / stage per group, the one radix
// sort, row pointer, row sums, output rows and offsets).  Internal to those two units: everything lives in an unnamed namespace, so
// each unit has kernels of its own.  What differs is a parameter: the factor on the coefficients ((1 - alpha) for PPR, none for
// Markov) and which of a tile's two copies is final (Tiles::fin).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_markov.h"
#include "rlap_ppr_tiles.h"
#include "rlap_snapshot.h"

namespace rlap {
namespace {

constexpr int PP_SMALL_THREADS = 512;   // small regime: 8 waves per tile
constexpr int PP_THREADS = 256;         // every other kernel
enum { PERR_WEIGHT = COL_ERR_WORDS, PERR_WORDS = 8 };
using pprtiles::T_SEG; using pprtiles::T_C0; using pprtiles::T_XOFF; using pprtiles::T_ROFF; using pprtiles::T_FIELDS;   // the tile table

__global__ void k_pp_weights(const double* __restrict__ sc, int64_t m, int zero_ok, int32_t* __restrict__ err) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const double w = sc[3 * r + 2];
    const bool ok = (zero_ok ? w >= 0.0 : w > 0.0) && w < INFINITY;
    if (!ok) atomicOr(&err[PERR_WEIGHT], 1);
}

// per block: D^-1/2 (0 for a zero degree, as the dense path) and the self loop's diagonal term scale / d (scaled: else rlap_markov.h's 1 / d)
__global__ void k_pp_degrees(const double* __restrict__ sc, const int32_t* __restrict__ bstart, int64_t B, int weighted, int self_loop,
                             int scaled, double scale, double* __restrict__ dinv, double* __restrict__ cdiag) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double d = 0.0;
    for (int32_t r = bstart[b]; r < bstart[b + 1]; ++r) d += weighted ? sc[3 * (int64_t)r + 2] : 1.0;
    if (self_loop) d += 1.0;
    const double di = markov::dinv(d);   // (d > 0 ? 1 / sqrt(d) : 0)
    dinv[b] = di;
    cdiag[b] = self_loop ? (scaled ? scale * (di * di) : markov::diag(di)) : 0.0;
}

// a_r = scale w_r D_b^-1/2 D_rb^-1/2 (scaled: else rlap_markov.h's coefficient, without the factor), once per row (blk: the inclusive scan of the block starts,
// block of row r = blk[r] - 1)
__global__ void k_pp_norm(const double* __restrict__ sc, int64_t m, int weighted, int scaled, double scale, const int32_t* __restrict__ blk,
                          const int32_t* __restrict__ rb, const double* __restrict__ dinv, double* __restrict__ a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= m) return;
    const double w = weighted ? sc[3 * r + 2] : 1.0;
    const double di = dinv[blk[r] - 1], dj = dinv[rb[r]];
    a[r] = scaled ? (scale * w) * (di * dj) : markov::coef(w, di, dj);
}

// block sort keys: (segment << 32) | id -- sorted, they give every block its rank among its segment's ids
__global__ void k_pp_bkeys(const double* __restrict__ sc, const int32_t* __restrict__ bstart, const int64_t* __restrict__ sb, int64_t S,
                           int64_t B, uint64_t* __restrict__ key, int32_t* __restrict__ val) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int64_t s = seg_of(sb, S, b);
    key[b] = ((uint64_t)s << 32) | (uint64_t)(int64_t)sc[3 * (int64_t)bstart[b] + 1];
    val[b] = (int32_t)b;
}

__global__ void k_pp_ranks(const uint64_t* __restrict__ key, const int32_t* __restrict__ pos_blk, const int64_t* __restrict__ sb, int64_t B,
                           int32_t* __restrict__ rank) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= B) return;
    rank[pos_blk[p]] = (int32_t)(p - sb[key[p] >> 32]);
}

struct Tiles {
    const int64_t* tab;       // [tiles][T_FIELDS]
    const double* om;         // PPR: [K] Chebyshev weights
    const double* sc; const int32_t* bstart; const int32_t* rb; const int64_t* sb; const double* a; const double* cdiag;
    const int32_t* rank;
    double* x;                // the tile area
    double alpha, eps;
    int32_t K;                // PPR: the Chebyshev steps; Markov: the order
    int32_t fin;              // which copy of a tile holds the result (0: the first, 1: the second)
};

// the kept entries of row q of a group in the final copy, counted (pass 0) or staged (pass 1) at top + (scan[q] - cnt[q]) + lane prefix
__global__ __launch_bounds__(PP_THREADS) void k_pp_keep(Tiles T, const int64_t* __restrict__ gt, int64_t nt, int64_t rows, int pass,
                                                        int32_t* __restrict__ cnt, const int64_t* __restrict__ scan,
                                                        const int64_t* __restrict__ top, uint64_t* __restrict__ key,
                                                        double* __restrict__ val, int64_t cap) {
    const int64_t q = (int64_t)blockIdx.x * (PP_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (q >= rows) return;
    int64_t lo = 0, hi = nt;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (T.tab[(gt[0] + mid) * T_FIELDS + T_ROFF] <= q) lo = mid; else hi = mid;
    }
    const int64_t* d = T.tab + (gt[0] + lo) * T_FIELDS;
    const int64_t s = d[T_SEG], c0 = d[T_C0];
    const int64_t b0 = T.sb[s], n = T.sb[s + 1] - b0;
    const int64_t i = q - d[T_ROFF];
    const int lane = threadIdx.x & 63;
    const double* xk = T.x + d[T_XOFF] + (T.fin ? n * PPR_TILE : 0);
    const int64_t src = c0 + lane;
    const int32_t ri = T.rank[b0 + i];
    const int32_t rj = src < n ? T.rank[b0 + src] : 0;
    const double v = src < n ? xk[i * PPR_TILE + lane] : 0.0;
    const bool keep = src < n && ri >= rj && v >= T.eps;
    const bool mirror = keep && ri != rj;
    const unsigned long long mk = __ballot(keep), mm = __ballot(mirror);
    if (pass == 0) {
        if (lane == 0) cnt[q] = __popcll(mk) + __popcll(mm);
        return;
    }
    if (!keep) return;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    int64_t o = top[0] + (scan[q] - cnt[q]) + __popcll(mk & below) + __popcll(mm & below);
    const uint64_t pi = (uint64_t)(b0 + ri), pj = (uint64_t)(b0 + rj);
    if (o < cap) { key[o] = (pi << 32) | (uint64_t)rj; val[o] = v; }
    if (mirror && o + 1 < cap) { key[o + 1] = (pj << 32) | (uint64_t)ri; val[o + 1] = v; }
}

__global__ void k_pp_top(int64_t* __restrict__ top, const int64_t* __restrict__ scan, int64_t rows) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && rows > 0) top[0] += scan[rows - 1];
}

// rowptr[p] = first sorted entry of position p (rows of positions without entries are empty)
__global__ void k_pp_rowptr(const uint64_t* __restrict__ key, int64_t P, int64_t B, int64_t* __restrict__ rowptr) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P) return;
    const int64_t p = (int64_t)(key[e] >> 32);
    const int64_t pp = e == 0 ? -1 : (int64_t)(key[e - 1] >> 32);
    for (int64_t u = pp + 1; u <= p; ++u) rowptr[u] = e;
    if (e == P - 1) for (int64_t u = p + 1; u <= B; ++u) rowptr[u] = P;
}

// D_S^-1/2 per position: one wave per row, lane strides then an xor butterfly (a fixed order)
__global__ __launch_bounds__(PP_THREADS) void k_pp_rowsum(const double* __restrict__ val, const int64_t* __restrict__ rowptr, int64_t B,
                                                          double* __restrict__ dsinv) {
    const int64_t p = (int64_t)blockIdx.x * (PP_THREADS / 64) + (threadIdx.x >> 6);
    if (p >= B) return;
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int64_t e = rowptr[p] + lane; e < rowptr[p + 1]; e += 64) acc += val[e];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) dsinv[p] = acc > 0.0 ? 1.0 / sqrt(acc) : 0.0;
}

__global__ void k_pp_out(const uint64_t* __restrict__ key, const double* __restrict__ val, int64_t P, const int64_t* __restrict__ sb,
                         int64_t S, const int32_t* __restrict__ pos_blk, const int32_t* __restrict__ bstart, const double* __restrict__ sc,
                         const double* __restrict__ dsinv, int normalize, double* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P) return;
    const int64_t p = (int64_t)(key[e] >> 32);
    const int64_t s = seg_of(sb, S, p);
    const int64_t pj = sb[s] + (int64_t)(key[e] & 0xffffffffull);
    const double v = val[e];
    out[3 * e] = sc[3 * (int64_t)bstart[pos_blk[p]] + 1];
    out[3 * e + 1] = sc[3 * (int64_t)bstart[pos_blk[pj]] + 1];
    out[3 * e + 2] = normalize ? v * (dsinv[p] * dsinv[pj]) : v;
}

__global__ void k_pp_outptr(const int64_t* __restrict__ sb, int64_t S, const int64_t* __restrict__ rowptr, int64_t* __restrict__ out_ptr) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s <= S) out_ptr[s] = rowptr[sb[s]];
}

struct Bufs {
    ColumnBufs col;
    double *dinv, *cdiag, *a, *dsinv, *x, *om, *vin, *vout;
    uint64_t *bkey, *bkey_out, *kin, *kout;
    int32_t *bval, *pos_blk, *rank, *cnt;
    int64_t *tab, *gt, *scan, *rowptr, *top, *nodes;
    void* tmp; size_t tmp_bytes;
    int64_t tcap, area, area_rows;
};

size_t carve_ppr(Carve& C, int64_t m, int64_t S, int64_t G, int64_t N, int64_t cap, int32_t K, Bufs& B) {
    C.off = column_pass_carve(C.base, C.off, m, S, G, N, PERR_WORDS, &B.col);
    const int64_t bc = B.col.bcap;
    const pprtiles::Sizes z = pprtiles::sizes(bc, S);   // (rlap_ppr_tiles.h)
    B.tcap = z.tcap;
    B.area = z.area;
    B.area_rows = z.area_rows;
    B.dinv = C.take<double>(bc);
    B.cdiag = C.take<double>(bc);
    B.a = C.take<double>(m);
    B.dsinv = C.take<double>(bc);
    B.bkey = C.take<uint64_t>(bc);
    B.bkey_out = C.take<uint64_t>(bc);
    B.bval = C.take<int32_t>(bc);
    B.pos_blk = C.take<int32_t>(bc);
    B.rank = C.take<int32_t>(bc);
    B.tab = C.take<int64_t>(T_FIELDS * B.tcap + B.tcap + 1);   // tiles, then the group starts
    B.gt = B.tab + T_FIELDS * B.tcap;
    B.om = C.take<double>(std::max<int32_t>(K, 1));
    B.cnt = C.take<int32_t>(B.area_rows);
    B.scan = C.take<int64_t>(B.area_rows);
    B.top = C.take<int64_t>(1);
    B.nodes = C.take<int64_t>(S);
    B.rowptr = C.take<int64_t>(bc + 1);
    B.kin = C.take<uint64_t>(cap);
    B.vin = C.take<double>(cap);
    B.kout = C.take<uint64_t>(cap);
    B.vout = C.take<double>(cap);
    size_t t1 = 0, t2 = 0, t3 = 0;
    (void)rocprim::radix_sort_pairs(nullptr, t1, (uint64_t*)nullptr, (uint64_t*)nullptr, (double*)nullptr, (double*)nullptr,
                                    (size_t)std::max<int64_t>(cap, 1), 0, 64, (hipStream_t)0);
    (void)rocprim::radix_sort_pairs(nullptr, t2, (uint64_t*)nullptr, (uint64_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr,
                                    (size_t)std::max<int64_t>(bc, 1), 0, 64, (hipStream_t)0);
    (void)rocprim::inclusive_scan(nullptr, t3, (const int32_t*)nullptr, (int64_t*)nullptr, (size_t)B.area_rows, rocprim::plus<int64_t>(),
                                  (hipStream_t)0);
    B.tmp_bytes = std::max(t1, std::max(t2, t3));
    B.tmp = C.take<char>((int64_t)B.tmp_bytes);
    B.x = C.take<double>(B.area);
    return C.off + 256;
}

int bits_for(int64_t v) { int b = 1; while (b < 62 && ((int64_t)1 << b) <= v) ++b; return b; }

// what a call knows after its prologue
struct Prologue {
    Bufs B;
    std::vector<int64_t> hnodes;   // nodes of every segment
    int64_t Btot = 0;              // blocks (nodes) of the call
    int32_t host_syncs = 0;
    bool done = false;             // m == 0: the offsets are written and nothing is left to do
};

// Steps 1 to 3 of a call: the tables, read back and checked; the arena carved; the column pass, the weights and the degrees, read
// back once; per block and per row the degrees, the coefficients (with the factor `scale` where `scaled`) and the ranks by id.
int pp_prologue(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotSeg& in, int64_t out_cap, int32_t K, int weighted, int self_loop,
                int zero_ok, int scaled, double scale, int64_t* out_ptr, Prologue* P) {
    const int64_t m = in.m, S = in.S, G = in.G, N = in.N;
    Bufs& B = P->B;
    // 1. the tables, read back and checked
    std::vector<int64_t> hptr, hnp;
    int rc = read_tables_checked(st, in.ptr, S, m, in.node_ptr, G, N, &hptr, &hnp);
    P->host_syncs = 1;
    if (rc != RLAP_OK) return rc;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_ppr(C, m, S, G, N, out_cap, K, B) > ws_bytes) return RLAP_E_WORKSPACE;
    if (m == 0) {
        RLAP_HIPCHK(hipMemsetAsync(out_ptr, 0, sizeof(int64_t) * (size_t)(S + 1), st));
        P->done = true;
        return RLAP_OK;
    }
    // 2. the column pass, the weights, the degrees, read back once
    RLAP_HIPCHK(hipMemsetAsync(B.col.err, 0, sizeof(int32_t) * PERR_WORDS, st));
    std::vector<int64_t>& hnodes = P->hnodes;
    hnodes.assign((size_t)S, 0);
    int64_t* d_nodes = B.nodes;
    rc = column_pass_enqueue(st, in.sc, m, in.ptr, S, in.node_ptr, G, N, B.col, d_nodes);
    if (rc != RLAP_OK) return rc;
    hipLaunchKernelGGL(k_pp_weights, dim3(grid_blocks(m, 256)), dim3(256), 0, st, in.sc, m, zero_ok, B.col.err);
    RLAP_HIPCHK(hipGetLastError());
    int32_t herr[PERR_WORDS];
    RLAP_HIPCHK(hipMemcpyAsync(hnodes.data(), d_nodes, sizeof(int64_t) * (size_t)S, hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipMemcpyAsync(herr, B.col.err, sizeof(herr), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    P->host_syncs += 1;
    rc = layout_status(herr);
    if (rc != RLAP_OK) return rc;
    if (weighted && herr[PERR_WEIGHT]) return RLAP_E_BAD_ARG;
    int64_t Btot = 0;
    for (int64_t s = 0; s < S; ++s) Btot += hnodes[(size_t)s];
    if (Btot > B.col.bcap) return RLAP_E_INTERNAL;
    P->Btot = Btot;
    // 3. per block and per row: degrees, normalised weights, ranks by id
    hipLaunchKernelGGL(k_pp_degrees, dim3(grid_blocks(Btot, 256)), dim3(256), 0, st, in.sc, B.col.bstart, Btot, weighted, self_loop, scaled, scale,
                       B.dinv, B.cdiag);
    hipLaunchKernelGGL(k_pp_norm, dim3(grid_blocks(m, 256)), dim3(256), 0, st, in.sc, m, weighted, scaled, scale, B.col.blk, B.col.rb, B.dinv, B.a);
    hipLaunchKernelGGL(k_pp_bkeys, dim3(grid_blocks(Btot, 256)), dim3(256), 0, st, in.sc, B.col.bstart, B.col.sb, S, Btot, B.bkey, B.bval);
    RLAP_HIPCHK(hipGetLastError());
    size_t tb = B.tmp_bytes;
    RLAP_HIPCHK(rocprim::radix_sort_pairs(B.tmp, tb, B.bkey, B.bkey_out, B.bval, B.pos_blk, (size_t)Btot, 0, 32 + bits_for(S), st));
    hipLaunchKernelGGL(k_pp_ranks, dim3(grid_blocks(Btot, 256)), dim3(256), 0, st, B.bkey_out, B.pos_blk, B.col.sb, Btot, B.rank);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// Step 4: the tile table `tt` checked against the arena and uploaded with its group starts; the output counter zeroed.
int pp_upload_table(hipStream_t st, pprtiles::Table& tt, const Prologue& P) {
    const Bufs& B = P.B;
    if (!pprtiles::fits(tt, pprtiles::Sizes{B.tcap, B.area, B.area_rows}, P.hnodes.data())) return RLAP_E_INTERNAL;
    const int64_t ntiles = tt.ntiles();
    std::vector<int64_t>& tab = tt.tab;
    tab.resize((size_t)(T_FIELDS * B.tcap), 0);
    for (int64_t g = 0; g < tt.ngroups(); ++g) tab.push_back(tt.gstart[(size_t)g]);
    tab.push_back(ntiles);
    RLAP_HIPCHK(hipMemcpyAsync(B.tab, tab.data(), sizeof(int64_t) * tab.size(), hipMemcpyHostToDevice, st));
    RLAP_HIPCHK(hipMemsetAsync(B.top, 0, sizeof(int64_t), st));
    return RLAP_OK;
}

// After a group's sweeps: its kept entries counted, scanned and staged behind those of the groups before (four launches).
int pp_group_keep(hipStream_t st, const Tiles& T, const Bufs& B, const int64_t* gt, int64_t nt, int64_t rows, int64_t out_cap) {
    hipLaunchKernelGGL(k_pp_keep, dim3(grid_blocks(rows, PP_THREADS / 64)), dim3(PP_THREADS), 0, st, T, gt, nt, rows, 0, B.cnt, B.scan,
                       B.top, B.kin, B.vin, out_cap);
    RLAP_HIPCHK(hipGetLastError());
    size_t sbytes = B.tmp_bytes;
    RLAP_HIPCHK(rocprim::inclusive_scan(B.tmp, sbytes, B.cnt, B.scan, (size_t)rows, rocprim::plus<int64_t>(), st));
    hipLaunchKernelGGL(k_pp_keep, dim3(grid_blocks(rows, PP_THREADS / 64)), dim3(PP_THREADS), 0, st, T, gt, nt, rows, 1, B.cnt, B.scan,
                       B.top, B.kin, B.vin, out_cap);
    hipLaunchKernelGGL(k_pp_top, dim3(1), dim3(64), 0, st, B.top, B.scan, rows);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

// Steps 6 and 7: the kept count, read back once (too many for the caller's buffer: nothing is written, the count is reported);
// then (segment, i, j) order, row sums, the output rows and offsets.
int pp_epilogue(hipStream_t st, const SnapshotSeg& in, Prologue* Pr, int normalize, double* out, int64_t out_cap, int64_t* out_ptr,
                int64_t* kept) {
    const Bufs& B = Pr->B;
    const int64_t S = in.S, Btot = Pr->Btot;
    int64_t P = 0;
    RLAP_HIPCHK(hipMemcpyAsync(&P, B.top, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipStreamSynchronize(st));
    Pr->host_syncs += 1;
    *kept = P;
    if (P > out_cap) return RLAP_E_OUT_CAPACITY;
    if (P > 0) {
        size_t tb = B.tmp_bytes;
        RLAP_HIPCHK(rocprim::radix_sort_pairs(B.tmp, tb, B.kin, B.kout, B.vin, B.vout, (size_t)P, 0, 32 + bits_for(Btot), st));
    }
    RLAP_HIPCHK(hipMemsetAsync(B.rowptr, 0, sizeof(int64_t) * (size_t)(Btot + 1), st));
    hipLaunchKernelGGL(k_pp_rowptr, dim3(grid_blocks(P, 256)), dim3(256), 0, st, B.kout, P, Btot, B.rowptr);
    hipLaunchKernelGGL(k_pp_rowsum, dim3(grid_blocks(Btot, PP_THREADS / 64)), dim3(PP_THREADS), 0, st, B.vout, B.rowptr, Btot, B.dsinv);
    hipLaunchKernelGGL(k_pp_out, dim3(grid_blocks(P, 256)), dim3(256), 0, st, B.kout, B.vout, P, B.col.sb, S, B.pos_blk, B.col.bstart, in.sc,
                       B.dsinv, normalize, out);
    hipLaunchKernelGGL(k_pp_outptr, dim3(grid_blocks(S + 1, 256)), dim3(256), 0, st, B.col.sb, S, B.rowptr, out_ptr);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace
}  // namespace rlap
