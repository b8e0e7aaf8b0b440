// rlap_probe.hip -- the linear-probe evaluator (rlap_linear_probe / rlap_probe_scores): R independent runs of
// LREvaluator's loop (scripts/node_shared.py:163-230) or of CCA-SSG/main.py:152-194's in one call, the scores computed on the
// device, nothing synchronised with the host.  Every value and the order of every sum are rlap_probe.h's.  A translation unit of
// its own.
//
//   start      the training rows of every run gathered once into a contiguous image (rows padded with zeros to 32-row tiles, row
//              stride F | 1 floats), their labels beside them; W copied, a transposed copy Wt (F, Cp) padded to Cp = 8 .. 64
//              classes for the kernels' coalesced reads; Adam's moments and the records zeroed.
//   epoch      k_probe_epoch, grid (parts, runs): a workgroup streams the 32-row tiles of its part through LDS, one read of a
//              training row per epoch.  Per tile: the logits as float32 fmaf chains over k (a thread owns one class and Cp / 8
//              rows, so a load of Wt serves Cp / 8 chains), the softmax of a row by one thread in the rule's order, g left in
//              LDS, then g^T x as fmaf chains over the rows (a thread owns up to two feature columns and all Cp classes in
//              registers).  Neither the logits nor g reach memory; a part writes one partial (C, F) and the chunk sums of db.
//              The chains are the rule's, bit for bit what the f32 matrix-core instruction forms; they run on the vector ALUs here,
//              because at these sizes (C <= 64) one accumulator tile per wave would leave the matrix cores no faster.
//   step       k_probe_step, all runs in one launch: the parts added in order in float64, Adam, W / Wt / b written.
//   scoring    k_probe_score over the validation and test lists of all runs (rows gathered through the lists, the same logits,
//              argmax's tie rule, integer atomics into the confusion counts), then k_probe_select, one workgroup per run: counts to
//              scores, the selection rule on a record in device memory.
// Ordering is stream order alone: no cooperative launch, no barrier or wait between workgroups.  No float atomics.  Every index read
// from a list is checked against [0, N) before it becomes an address.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>

#include "../../include/rlap_hip.h"
#include "rlap_probe.h"
#include "rlap_probe_api.h"
#include "rlap_spmm.h"

namespace rlap {
namespace {

static_assert(probe::STATUS_INDEX == RLAP_E_INDEX_RANGE && probe::STATUS_LABEL == RLAP_E_BAD_ARG, "the status word holds RLAP codes");

constexpr int PB_THREADS = 256;
constexpr int64_t PB_MAX_GRID = 1 << 16;

// the runs' tables, passed by value: image rows, chunks and list offsets
struct Runs {
    int64_t row0[probe::MAX_RUNS + 1];     // first row of run r's training image (padded rows before it)
    int64_t chunk0[probe::MAX_RUNS + 1];   // first chunk of run r's training list
    int64_t off[3][probe::MAX_RUNS + 1];   // the offsets of the training, validation and test lists
};

struct Dev {
    const float* x; int64_t N, ldx; const int64_t* y; int F, C, CP, LS, R, PS;   // PS: parts of the partial sums' layout (the largest of the runs)
    const int64_t* idx[3];
    float* ximg; int32_t* yimg;            // the training images and their labels (-1: outside [0, C))
    float* w; float* b; float* wt; float* bt;   // (R, C, F), (R, C); (R, F, CP), (R, CP)
    float* mom;                            // (R, 2, C F + C): Adam's m and v
    float* partial;                        // (R, PS, C, F)
    double* bchunk;                        // (chunks, C): the chunk sums of db
    double* lossrow; double* lchunk;       // (image rows), (chunks)
    int32_t* count;                        // (R, 2, C, C): the working confusion counts
    probe::Record* rec;                    // (R)
    int32_t* status;
    double* scores; int64_t* best; int64_t* confusion; int64_t* pred;
};

__device__ inline void raise(int32_t* status, int code) { atomicMax(status, code); }

// a list's index, checked: row 0 stands in for one outside [0, N)
__device__ inline int64_t checked_index(const Dev& d, const int64_t* list, int64_t i) {
    const int64_t v = list[i];
    if (v < 0 || v >= d.N) { raise(d.status, probe::STATUS_INDEX); return 0; }
    return v;
}
__device__ inline int32_t checked_label(const Dev& d, int64_t row) {
    const int64_t v = d.y[row];
    if (v < 0 || v >= d.C) { raise(d.status, probe::STATUS_LABEL); return -1; }
    return (int32_t)v;
}

// ------------------------------------------------------------------------------------------------ start
__global__ __launch_bounds__(PB_THREADS) void k_probe_gather(Dev d, Runs t) {
    const int r = blockIdx.y;
    const int64_t n = t.off[0][r + 1] - t.off[0][r], np = probe::padded_rows(n);
    const int64_t* list = d.idx[0] + t.off[0][r];
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < np * d.LS; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / d.LS;
        const int k = (int)(e - i * d.LS);
        float val = 0.0f;
        if (i < n) {
            const int64_t row = checked_index(d, list, i);
            if (k < d.F) val = d.x[row * d.ldx + k];
            if (k == 0) d.yimg[t.row0[r] + i] = checked_label(d, row);
        } else if (k == 0) {
            d.yimg[t.row0[r] + i] = -1;
        }
        d.ximg[(t.row0[r] + i) * d.LS + k] = val;
    }
}

// W, b, Wt, bt from the initial parameters; the moments, the records, the counts and the results' initial values
__global__ __launch_bounds__(PB_THREADS) void k_probe_init(Dev d, const float* __restrict__ w0, const float* __restrict__ b0) {
    const int r = blockIdx.y;
    const int64_t cf = (int64_t)d.C * d.F, per = cf + d.C;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = tid; e < (int64_t)d.F * d.CP; e += stride) {
        const int k = (int)(e / d.CP), c = (int)(e - (int64_t)k * d.CP);
        d.wt[(int64_t)r * d.F * d.CP + e] = c < d.C ? w0[r * cf + (int64_t)c * d.F + k] : 0.0f;
    }
    for (int64_t e = tid; e < cf; e += stride) d.w[r * cf + e] = w0[r * cf + e];
    for (int64_t e = tid; e < d.CP; e += stride) d.bt[r * d.CP + e] = e < d.C ? b0[r * d.C + e] : 0.0f;
    for (int64_t e = tid; e < d.C; e += stride) d.b[r * d.C + e] = b0[r * d.C + e];
    if (d.mom)
        for (int64_t e = tid; e < 2 * per; e += stride) d.mom[r * 2 * per + e] = 0.0f;
    const int64_t cc = (int64_t)d.C * d.C, sets = d.rec ? 2 : 1;
    for (int64_t e = tid; e < sets * cc; e += stride) { d.count[r * sets * cc + e] = 0; d.confusion[r * sets * cc + e] = 0; }
    if (tid == 0) {
        if (d.rec) {
            d.rec[r] = probe::Record{0, 0, 0, 0};
            for (int j = 0; j < 4; ++j) d.scores[r * 4 + j] = 0.0;
            d.best[r * 2] = 0; d.best[r * 2 + 1] = 0;
        }
        if (r == 0) *d.status = probe::STATUS_OK;
    }
}

// ------------------------------------------------------------------------------------------------ the logits of a 32-row tile
// xs: 32 rows of LS floats in LDS; zs: 32 rows of CP + 1 floats in LDS.  Thread (c = tid % CP, tid / CP) owns class c of NJ rows.
template <int CP>
__device__ inline void tile_logits(const float* xs, int LS, const float* __restrict__ wt, const float* __restrict__ bt, int F, float* zs) {
    constexpr int NJ = CP / 8, RG = PB_THREADS / CP;   // rows of a thread; row groups: RG * NJ == 32
    const int c = threadIdx.x % CP, rg = threadIdx.x / CP;
    float acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = 0.0f;
    const float* xr = xs + rg * LS;
    for (int k = 0; k < F; ++k) {
        const float wv = wt[(int64_t)k * CP + c];
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[j] = probe::chain_step(acc[j], xr[j * RG * LS + k], wv);
    }
    const float bias = bt[c];
#pragma unroll
    for (int j = 0; j < NJ; ++j) zs[(rg + j * RG) * (CP + 1) + c] = probe::logit_of(bias, acc[j]);
}

// ------------------------------------------------------------------------------------------------ the epoch
template <int CP, int KA>
__global__ __launch_bounds__(PB_THREADS) void k_probe_epoch(Dev d, Runs t) {
    extern __shared__ __attribute__((aligned(16))) float pb_lds[];
    float* xs = pb_lds;                                  // 32 x LS
    float* zs = xs + probe::TILE * d.LS;                 // 32 x (CP + 1)
    int32_t* ys = reinterpret_cast<int32_t*>(zs + probe::TILE * (CP + 1));   // 32
    const int r = blockIdx.y, p = blockIdx.x, tid = threadIdx.x;
    const int64_t n = t.off[0][r + 1] - t.off[0][r];
    if (p >= probe::num_parts(n, d.F, d.C)) return;      // (uniform)
    const int64_t rb = probe::part_begin(n, d.F, d.C, p), re = probe::part_end(n, d.F, d.C, p);
    const float* __restrict__ wt = d.wt + (int64_t)r * d.F * CP;
    const float* __restrict__ bt = d.bt + (int64_t)r * CP;
    const float* __restrict__ img = d.ximg + t.row0[r] * d.LS;
    const int32_t* __restrict__ yimg = d.yimg + t.row0[r];

    float acc[KA][CP];
#pragma unroll
    for (int a = 0; a < KA; ++a)
#pragma unroll
        for (int c = 0; c < CP; ++c) acc[a][c] = 0.0f;
    double bsum = 0.0;                                   // thread c < C: the running chunk sum of db_c

#pragma unroll 1
    for (int64_t row0 = rb; row0 < re; row0 += probe::TILE) {   // (rb is a multiple of 256; the image holds whole tiles)
        const int nrows = re - row0 < probe::TILE ? (int)(re - row0) : probe::TILE;
        __syncthreads();                                 // (the previous tile has been read)
        for (int j = tid; j < probe::TILE * d.LS; j += PB_THREADS) xs[j] = img[row0 * d.LS + j];
        if (tid < probe::TILE) ys[tid] = yimg[row0 + tid];
        __syncthreads();
        tile_logits<CP>(xs, d.LS, wt, bt, d.F, zs);
        __syncthreads();
        if (tid < probe::TILE) {
            float* z = zs + tid * (CP + 1);
            if (tid < nrows) d.lossrow[t.row0[r] + row0 + tid] = probe::row_softmax(z, d.C, ys[tid]);
        }
        __syncthreads();
        if (tid < d.C) {
            for (int i = 0; i < nrows; ++i) bsum = spmm::accumulate(bsum, 1.0, (double)zs[i * (CP + 1) + tid]);
            const int64_t next = row0 + probe::TILE;
            if (next % spmm::CHUNK == 0 || next >= re) {   // the chunk ends with this tile
                d.bchunk[(t.chunk0[r] + row0 / spmm::CHUNK) * d.C + tid] = bsum;
                bsum = 0.0;
            }
        }
#pragma unroll
        for (int a = 0; a < KA; ++a) {
            const int k = tid + a * PB_THREADS;
            if (k < d.F) {
                for (int i = 0; i < nrows; ++i) {
                    const float xv = xs[i * d.LS + k];
                    const float* g = zs + i * (CP + 1);
#pragma unroll
                    for (int c = 0; c < CP; ++c) acc[a][c] = probe::chain_step(acc[a][c], g[c], xv);
                }
            }
        }
    }

    float* __restrict__ out = d.partial + ((int64_t)r * d.PS + p) * d.C * d.F;
#pragma unroll
    for (int a = 0; a < KA; ++a) {
        const int k = tid + a * PB_THREADS;
        if (k < d.F) {
#pragma unroll
            for (int c = 0; c < CP; ++c)
                if (c < d.C) out[(int64_t)c * d.F + k] = acc[a][c];
        }
    }
}

// ------------------------------------------------------------------------------------------------ the step
__global__ __launch_bounds__(PB_THREADS) void k_probe_step(Dev d, Runs t, probe::AdamCoef coef) {
    const int r = blockIdx.y;
    const int64_t n = t.off[0][r + 1] - t.off[0][r];
    const int64_t cf = (int64_t)d.C * d.F, per = cf + d.C;
    const int parts = (int)probe::num_parts(n, d.F, d.C);
    float* m = d.mom + (int64_t)r * 2 * per;
    float* v = m + per;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < per; e += (int64_t)gridDim.x * blockDim.x) {
        if (e < cf) {
            const int c = (int)(e / d.F), k = (int)(e - (int64_t)c * d.F);
            const float* __restrict__ part = d.partial + (int64_t)r * d.PS * cf + e;
            double total = 0.0;
            for (int p = 0; p < parts; ++p) total = total + (double)part[(int64_t)p * cf];
            float w = d.w[r * cf + e];
            probe::adam_step(coef, probe::mean_grad(total, n), &w, &m[e], &v[e]);
            d.w[r * cf + e] = w;
            d.wt[((int64_t)r * d.F + k) * d.CP + c] = w;
        } else {
            const int c = (int)(e - cf);
            const int64_t nc = spmm::num_chunks(n);
            double total = 0.0;
            for (int64_t q = 0; q < nc; ++q) total = total + d.bchunk[(t.chunk0[r] + q) * d.C + c];
            float b = d.b[r * d.C + c];
            probe::adam_step(coef, probe::mean_grad(total, n), &b, &m[e], &v[e]);
            d.b[r * d.C + c] = b;
            d.bt[r * d.CP + c] = b;
        }
    }
}

// ------------------------------------------------------------------------------------------------ scoring
// grid (tiles, runs, sets): set s of the launch is list first_set + s; counts are (R, sets, C, C)
template <int CP>
__global__ __launch_bounds__(PB_THREADS) void k_probe_score(Dev d, Runs t, int first_set) {
    extern __shared__ __attribute__((aligned(16))) float pb_lds[];
    float* xs = pb_lds;
    float* zs = xs + probe::TILE * d.LS;
    int32_t* ys = reinterpret_cast<int32_t*>(zs + probe::TILE * (CP + 1));
    int64_t* rows = reinterpret_cast<int64_t*>(ys + probe::TILE);   // (32 LS + 32 (CP + 1) + 32 floats: a multiple of 8 bytes)
    const int r = blockIdx.y, s = blockIdx.z, set = first_set + s, tid = threadIdx.x;
    const int64_t len = t.off[set][r + 1] - t.off[set][r], row0 = (int64_t)blockIdx.x * probe::TILE;
    if (row0 >= len) return;                             // (uniform)
    const int64_t* list = d.idx[set] + t.off[set][r];
    const int nrows = len - row0 < probe::TILE ? (int)(len - row0) : probe::TILE;
    if (tid < probe::TILE) {
        int64_t row = 0;
        int32_t lab = -1;
        if (tid < nrows) { row = checked_index(d, list, row0 + tid); lab = checked_label(d, row); }
        rows[tid] = row; ys[tid] = lab;
    }
    __syncthreads();
    for (int j = tid; j < probe::TILE * d.LS; j += PB_THREADS) {
        const int i = j / d.LS, k = j - i * d.LS;
        xs[j] = (i < nrows && k < d.F) ? d.x[rows[i] * d.ldx + k] : 0.0f;
    }
    __syncthreads();
    tile_logits<CP>(xs, d.LS, d.wt + (int64_t)r * d.F * CP, d.bt + (int64_t)r * CP, d.F, zs);
    __syncthreads();
    if (tid < nrows) {
        const int pred = probe::predict(zs + tid * (CP + 1), d.C);
        if (d.pred) d.pred[t.off[set][r] + row0 + tid] = pred;
        if (ys[tid] >= 0) atomicAdd(&d.count[(((int64_t)r * gridDim.z + s) * d.C + ys[tid]) * d.C + pred], 1);
    }
}

// one workgroup per run: the counts of this evaluation to scores, the selection rule, the counts zeroed for the next one
__global__ __launch_bounds__(PB_THREADS) void k_probe_select(Dev d, Runs t, int select, int64_t epoch) {
    __shared__ int32_t cnt[2 * probe::MAX_C * probe::MAX_C];
    __shared__ double f1[probe::MAX_C];
    __shared__ int take;
    const int r = blockIdx.x, tid = threadIdx.x;
    const int cc = d.C * d.C;
    int32_t* src = d.count + (int64_t)r * 2 * cc;
    for (int e = tid; e < 2 * cc; e += PB_THREADS) { cnt[e] = src[e]; src[e] = 0; }
    __syncthreads();
    if (tid == 0) {
        probe::Record rec = d.rec[r];
        take = probe::select_take(select, probe::correct_of(cnt, d.C), probe::correct_of(cnt + cc, d.C), epoch, &rec) ? 1 : 0;
        d.rec[r] = rec;
    }
    __syncthreads();
    if (!take) return;                                   // (uniform)
    for (int e = tid; e < 2 * cc; e += PB_THREADS) d.confusion[(int64_t)r * 2 * cc + e] = cnt[e];
    if (tid < d.C) {                                     // the label's term of the macro mean, or -1 where the label does not occur
        int64_t rs = 0, cs = 0;
        for (int j = 0; j < d.C; ++j) { rs += cnt[cc + tid * d.C + j]; cs += cnt[cc + j * d.C + tid]; }
        f1[tid] = rs + cs > 0 ? probe::f1_of(cnt[cc + tid * d.C + tid], rs, cs) : -1.0;
    }
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
        int64_t present = 0;
        for (int c = 0; c < d.C; ++c)
            if (f1[c] >= 0.0) { total = total + f1[c]; ++present; }
        const int64_t rows = t.off[2][r + 1] - t.off[2][r];
        const double acc = (double)probe::correct_of(cnt + cc, d.C) / (double)rows;
        d.scores[r * 4 + 0] = acc;
        d.scores[r * 4 + 1] = present > 0 ? total / (double)present : 0.0;
        d.scores[r * 4 + 2] = acc;
    }
}

// the scoring pass alone: counts to the (R, C, C) matrices and the (R, 3) scores
__global__ __launch_bounds__(64) void k_probe_scores_finish(Dev d, Runs t) {
    const int r = blockIdx.x;
    const int cc = d.C * d.C;
    for (int e = threadIdx.x; e < cc; e += blockDim.x) d.confusion[(int64_t)r * cc + e] = d.count[(int64_t)r * cc + e];
    if (threadIdx.x == 0)
        probe::scores_of(d.count + (int64_t)r * cc, d.C, t.off[0][r + 1] - t.off[0][r], &d.scores[r * 3], &d.scores[r * 3 + 1], &d.scores[r * 3 + 2]);
}

// ------------------------------------------------------------------------------------------------ the end of the call
__global__ __launch_bounds__(PB_THREADS) void k_probe_losschunks(Dev d, Runs t) {
    const int r = blockIdx.y;
    const int64_t n = t.off[0][r + 1] - t.off[0][r], nc = spmm::num_chunks(n);
    const double* rows = d.lossrow + t.row0[r];
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nc; q += (int64_t)gridDim.x * blockDim.x)
        d.lchunk[t.chunk0[r] + q] = spmm::chunk_sum(n, q, [](int64_t) { return 1.0; }, [&](int64_t i) { return rows[i]; });
}

__global__ __launch_bounds__(64) void k_probe_finish(Dev d, Runs t) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= d.R) return;
    const int64_t n = t.off[0][r + 1] - t.off[0][r], nc = spmm::num_chunks(n);
    double total = 0.0;
    for (int64_t q = 0; q < nc; ++q) total = total + d.lchunk[t.chunk0[r] + q];
    d.scores[r * 4 + 3] = total / (double)n;
    d.best[r * 2] = d.rec[r].epoch;
    d.best[r * 2 + 1] = d.rec[r].best_val;
}

// ------------------------------------------------------------------------------------------------ host
bool fill_runs(const ProbeArgs& a, int nlists, Runs* t, int64_t* max_parts, int64_t* max_tiles) {
    *t = Runs{};
    *max_parts = 1; *max_tiles = 1;
    for (int s = 0; s < nlists; ++s) {
        if (!probe_lists_ok(a.hptr[s], a.R)) return false;
        for (int64_t r = 0; r <= a.R; ++r) t->off[s][r] = a.hptr[s][r];
    }
    for (int64_t r = 0; r < a.R; ++r) {
        const int64_t n = t->off[0][r + 1] - t->off[0][r];
        t->row0[r + 1] = t->row0[r] + probe::padded_rows(n);
        t->chunk0[r + 1] = t->chunk0[r] + spmm::num_chunks(n);
        *max_parts = std::max(*max_parts, probe::num_parts(n, a.F, a.C));
        for (int s = nlists == 1 ? 0 : 1; s < nlists; ++s)
            *max_tiles = std::max(*max_tiles, probe::num_tiles(t->off[s][r + 1] - t->off[s][r]));
    }
    return true;
}

size_t carve_probe(Carve& K, const ProbeArgs& a, const Runs& t, int64_t max_parts, bool train, Dev* d) {
    const int CP = probe::class_pad(a.C);
    const int64_t R = a.R, cf = a.C * a.F;
    *d = Dev{};
    d->x = a.x; d->N = a.N; d->ldx = a.ldx; d->y = a.y; d->F = (int)a.F; d->C = (int)a.C; d->CP = CP; d->LS = (int)probe::image_stride(a.F);
    d->R = (int)R; d->PS = (int)max_parts;
    for (int s = 0; s < 3; ++s) d->idx[s] = a.idx[s];
    d->wt = K.take<float>(R * a.F * CP);
    d->bt = K.take<float>(R * CP);
    d->count = K.take<int32_t>(R * (train ? 2 : 1) * a.C * a.C);
    if (train) {
        d->ximg = K.take<float>(t.row0[R] * d->LS);
        d->yimg = K.take<int32_t>(t.row0[R]);
        d->mom = K.take<float>(R * 2 * (cf + a.C));
        d->partial = K.take<float>(R * max_parts * cf);
        d->bchunk = K.take<double>(t.chunk0[R] * a.C);
        d->lossrow = K.take<double>(t.row0[R]);
        d->lchunk = K.take<double>(t.chunk0[R]);
        d->rec = K.take<probe::Record>(R);
        d->w = a.w; d->b = a.b;
    } else {
        d->w = K.take<float>(R * cf);      // (k_probe_init's plain copies: the call's parameters are only read)
        d->b = K.take<float>(R * a.C);
    }
    d->status = a.status; d->scores = a.scores; d->best = a.best; d->confusion = a.confusion; d->pred = a.pred;
    return K.off + 256;
}

size_t lds_bytes(const Dev& d) { return (size_t)(probe::TILE * d.LS + probe::TILE * (d.CP + 1) + probe::TILE) * 4 + probe::TILE * 8; }

template <int CP, int KA>
int launch_epoch(hipStream_t st, const Dev& d, const Runs& t, int64_t max_parts, bool first) {
    const size_t lds = lds_bytes(d);
    if (first) RLAP_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_probe_epoch<CP, KA>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_probe_epoch<CP, KA>), dim3((unsigned)max_parts, (unsigned)d.R), dim3(PB_THREADS), lds, st, d, t);
    return RLAP_OK;
}
template <int CP>
int launch_epoch_cp(hipStream_t st, const Dev& d, const Runs& t, int64_t max_parts, bool first) {
    return d.F <= PB_THREADS ? launch_epoch<CP, 1>(st, d, t, max_parts, first) : launch_epoch<CP, 2>(st, d, t, max_parts, first);
}
int launch_epoch_any(hipStream_t st, const Dev& d, const Runs& t, int64_t max_parts, bool first) {
    return d.CP == 8 ? launch_epoch_cp<8>(st, d, t, max_parts, first) : d.CP == 16 ? launch_epoch_cp<16>(st, d, t, max_parts, first)
         : d.CP == 32 ? launch_epoch_cp<32>(st, d, t, max_parts, first) : launch_epoch_cp<64>(st, d, t, max_parts, first);
}

template <int CP>
int launch_score(hipStream_t st, const Dev& d, const Runs& t, int64_t max_tiles, int first_set, int sets, bool first) {
    const size_t lds = lds_bytes(d);
    if (first) RLAP_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_probe_score<CP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_probe_score<CP>), dim3((unsigned)max_tiles, (unsigned)d.R, (unsigned)sets), dim3(PB_THREADS), lds, st, d, t, first_set);
    return RLAP_OK;
}
int launch_score_any(hipStream_t st, const Dev& d, const Runs& t, int64_t max_tiles, int first_set, int sets, bool first) {
    return d.CP == 8 ? launch_score<8>(st, d, t, max_tiles, first_set, sets, first) : d.CP == 16 ? launch_score<16>(st, d, t, max_tiles, first_set, sets, first)
         : d.CP == 32 ? launch_score<32>(st, d, t, max_tiles, first_set, sets, first) : launch_score<64>(st, d, t, max_tiles, first_set, sets, first);
}

unsigned pb_blocks(int64_t n) { return capped_blocks(n, PB_THREADS, PB_MAX_GRID); }

}  // namespace

bool probe_lists_ok(const int64_t* hptr, int64_t R) {
    if (!hptr || hptr[0] != 0) return false;
    for (int64_t r = 0; r < R; ++r)
        if (hptr[r + 1] <= hptr[r] || hptr[r + 1] - hptr[r] >= (int64_t)1 << 31) return false;
    return true;
}

size_t probe_bytes(const ProbeArgs& a) {
    Runs t; Dev d; int64_t mp, mt;
    if (!fill_runs(a, 3, &t, &mp, &mt)) return 0;
    Carve K{nullptr, 0};
    return carve_probe(K, a, t, mp, true, &d);
}

size_t scores_bytes(const ProbeArgs& a) {
    Runs t; Dev d; int64_t mp, mt;
    if (!fill_runs(a, 1, &t, &mp, &mt)) return 0;
    Carve K{nullptr, 0};
    return carve_probe(K, a, t, mp, false, &d);
}

int probe_run(hipStream_t st, void* ws, size_t ws_bytes, const ProbeArgs& a, int64_t* parts, int64_t* launches) {
    Runs t; Dev d; int64_t max_parts, max_tiles;
    if (!fill_runs(a, 3, &t, &max_parts, &max_tiles)) return RLAP_E_BAD_ARG;
    Carve K{static_cast<char*>(ws), 0};
    if (carve_probe(K, a, t, max_parts, true, &d) > ws_bytes) return RLAP_E_WORKSPACE;
    const int64_t per = a.C * a.F + a.C;
    int64_t count = 0;
    int64_t max_img = 1;
    for (int64_t r = 0; r < a.R; ++r) max_img = std::max(max_img, (t.row0[r + 1] - t.row0[r]) * d.LS);
    hipLaunchKernelGGL(k_probe_init, dim3(pb_blocks(std::max<int64_t>(2 * per, a.F * d.CP)), (unsigned)a.R), dim3(PB_THREADS), 0, st, d, a.w0, a.b0);
    hipLaunchKernelGGL(k_probe_gather, dim3(pb_blocks(max_img), (unsigned)a.R), dim3(PB_THREADS), 0, st, d, t);
    RLAP_HIPCHK(hipGetLastError());
    count += 2;
    probe::AdamCoef coef;
    coef.init(a.lr, a.wd, a.beta1, a.beta2, a.eps);
    bool first_score = true;
    for (int64_t e = 0; e < a.epochs; ++e) {
        coef.advance();
        if (const int rc = launch_epoch_any(st, d, t, max_parts, e == 0)) return rc;
        hipLaunchKernelGGL(k_probe_step, dim3(pb_blocks(per), (unsigned)a.R), dim3(PB_THREADS), 0, st, d, t, coef);
        count += 2;
        if (probe::scoring_epoch(a.select, e, a.test_interval)) {
            if (const int rc = launch_score_any(st, d, t, max_tiles, 1, 2, first_score)) return rc;
            hipLaunchKernelGGL(k_probe_select, dim3((unsigned)a.R), dim3(PB_THREADS), 0, st, d, t, a.select, e);
            first_score = false;
            count += 2;
        }
        if ((e & 63) == 63) RLAP_HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_probe_losschunks, dim3(pb_blocks(std::max<int64_t>(1, max_img / d.LS / spmm::CHUNK)), (unsigned)a.R), dim3(PB_THREADS), 0, st, d, t);
    hipLaunchKernelGGL(k_probe_finish, dim3((unsigned)((a.R + 63) / 64)), dim3(64), 0, st, d, t);
    RLAP_HIPCHK(hipGetLastError());
    count += 2;
    if (parts) *parts = max_parts;
    if (launches) *launches = count;
    return RLAP_OK;
}

int scores_run(hipStream_t st, void* ws, size_t ws_bytes, const ProbeArgs& a, int64_t* launches) {
    Runs t; Dev d; int64_t max_parts, max_tiles;
    if (!fill_runs(a, 1, &t, &max_parts, &max_tiles)) return RLAP_E_BAD_ARG;
    Carve K{static_cast<char*>(ws), 0};
    if (carve_probe(K, a, t, max_parts, false, &d) > ws_bytes) return RLAP_E_WORKSPACE;
    hipLaunchKernelGGL(k_probe_init, dim3(pb_blocks(std::max<int64_t>(a.C * a.F, a.F * d.CP)), (unsigned)a.R), dim3(PB_THREADS), 0, st, d, a.w0, a.b0);
    RLAP_HIPCHK(hipGetLastError());
    if (const int rc = launch_score_any(st, d, t, max_tiles, 0, 1, true)) return rc;
    hipLaunchKernelGGL(k_probe_scores_finish, dim3((unsigned)a.R), dim3(64), 0, st, d, t);
    RLAP_HIPCHK(hipGetLastError());
    if (launches) *launches = 3;
    return RLAP_OK;
}

}  // namespace rlap
