// rlap_readout.hip -- per-graph readout of batched node embeddings (rlap_graph_readout / _backward): y[l, g, :] = the sum
// (or mean) of x[l, i, :] over the ids i of graph g, [node_ptr[g], node_ptr[g+1]), in the fixed order of rlap_spmm.h -- what
// global_add_pool(z, batch) does after every GIN layer, without float atomics.  A translation unit of its own.
//
//   counts   per graph (ranges clamped into [0, N), rlap_readout.h): its chunks, and its chunks when it is longer than one chunk;
//            two scans number the chunks of the call and the slots of the arena.  The host never reads them: the grid is sized
//            from the bound ceil(N / CHUNK) + G, and the kernels stride to the count they read on the device.
//   chunks   one work item per (layer, chunk, feature tile); lanes run along F, 16 bytes a lane where F allows, and a lane sums its
//            columns of the chunk's rows from 0 in id order (spmm::accumulate with coefficient 1.0).
//              wide   a row takes more than 32 lanes: one wave per item, eight rows of x in flight before the eight dependent adds.
//              narrow a row takes P <= 32 lanes: a wave takes 64 / P consecutive chunks.  Their rows are read in pieces of RO_R rows,
//                     every piece a contiguous span read by the whole wave 16 bytes (or one element) a lane, through LDS; then the
//                     P lanes of a chunk walk its piece there.  No lane strides through global memory by a chunk.
//            A graph of at most CHUNK ids is finished here (0 + its chunk sum, the division, the rounding); a longer one leaves
//            its chunk sums in the arena.
//   finish   per (layer, graph, column): an empty graph gets 0; a long one the sum of its chunk sums in chunk order.
// So every element of y is written, and its bits depend on the graph's own rows alone.  The backward call is one gather:
// gx[l, i, :] = gy[l, g(i), :] (mean: divided by the count in float64), g(i) by the segment search of rlap_snapshot.h.
// What is read from node_ptr is clamped before it is used as an address.  No atomic touches a floating-point value.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_readout.h"
#include "rlap_readout_api.h"
#include "rlap_spmm.h"

namespace rlap {
namespace {

constexpr int RO_THREADS = 256;
constexpr int RO_WAVES = RO_THREADS / 64;
constexpr int RO_R = 8;                                   // rows of a piece (narrow rows)
constexpr int RO_DEPTH = 8;                               // rows in flight (wide rows)
constexpr int RO_TILE_BYTES = 64 * 16 * RO_R + 64 * 16;   // a wave's pieces: 64 lanes x 16 bytes x RO_R rows, one unit of padding a chunk
constexpr int64_t RO_MAX_GRID = 8192;                     // workgroups of a launch (the kernels stride over their items)

inline unsigned ro_blocks(int64_t n, int per_block) { return capped_blocks(n, per_block, RO_MAX_GRID); }

// what the kernels share
struct Ro {
    const int64_t* np; int64_t N, G, L, F;
    int mean;
    int32_t* nch; int32_t* lch;               // [G+1] chunks of a graph; of a graph longer than one chunk (0 behind the last)
    int64_t* choff; int64_t* poff;            // [G+1] their exclusive scans
    double* part; int64_t pcap;               // [L, pcap, F] chunk sums of the long graphs
    int lg; int64_t ftiles;                   // log2 of the lanes of a row's group; groups a row of F features takes
};

template <class T, int VEC> __device__ inline void ro_load(const T* __restrict__ p, T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        v[0] = p[0];
    } else if constexpr (sizeof(T) == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        const double2 q = *reinterpret_cast<const double2*>(p);
        v[0] = q.x; v[1] = q.y;
    }
}

template <class T, int VEC> __device__ inline void ro_store(T* __restrict__ p, const T (&v)[VEC]) {
    if constexpr (VEC == 1) {
        p[0] = v[0];
    } else if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]);
    }
}

__global__ void k_ro_counts(Ro a) {
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g <= a.G; g += (int64_t)gridDim.x * blockDim.x) {
        int64_t s = 0, n = 0;
        if (g < a.G) readout::graph_range(a.np, g, a.N, &s, &n);
        a.nch[g] = readout::graph_chunks(n);
        a.lch[g] = readout::graph_part_chunks(n);
    }
}

// chunk k of graph g (n ids), layer l, columns [f0, f0 + VEC): its sum is `acc`
template <class T, int VEC>
__device__ inline void ro_emit(const Ro& a, int64_t l, int64_t g, int64_t k, int64_t n, int64_t f0, const double (&acc)[VEC], T* __restrict__ y) {
    if (n <= spmm::CHUNK) {   // the whole rule: 0 + the one chunk sum
        T out[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) out[v] = (T)readout::finish(0.0 + acc[v], n, a.mean != 0);
        ro_store<T, VEC>(y + (l * a.G + g) * a.F + f0, out);
        return;
    }
    const int64_t slot = a.poff[g] + k;
    if (slot < 0 || slot >= a.pcap) return;   // (only a table that is not well formed)
    double* __restrict__ p = a.part + (l * a.pcap + slot) * a.F + f0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) p[v] = acc[v];
}

// rows that take more than 32 lanes: one wave per (layer, chunk, feature tile)
template <class T, int VEC>
__global__ __launch_bounds__(RO_THREADS) void k_ro_wide(Ro a, const T* __restrict__ x, T* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int64_t total = a.choff[a.G];
    const int64_t items = a.L * total * a.ftiles;
    for (int64_t w = ((int64_t)blockIdx.x * RO_THREADS + threadIdx.x) >> 6; w < items; w += (int64_t)gridDim.x * RO_WAVES) {
        const int64_t lq = w / a.ftiles, ft = w - lq * a.ftiles;
        const int64_t l = lq / total, q = lq - l * total;
        const int64_t f0 = (ft * 64 + lane) * VEC;
        int64_t g = 0, k = 0, s = 0, n = 0;
        if (f0 >= a.F || !readout::item_of(a.choff, a.G, q, &g, &k)) continue;
        readout::graph_range(a.np, g, a.N, &s, &n);
        const int64_t cnt = spmm::chunk_end(n, k) - spmm::chunk_begin(k);
        if (cnt <= 0) continue;
        const T* __restrict__ xr = x + (l * a.N + s + spmm::chunk_begin(k)) * a.F + f0;
        double acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
        for (int64_t r = 0; r < cnt; r += RO_DEPTH) {
            T xv[RO_DEPTH][VEC];
#pragma unroll
            for (int u = 0; u < RO_DEPTH; ++u) ro_load<T, VEC>(xr + (r + u < cnt ? r + u : cnt - 1) * a.F, xv[u]);   // (a turn past the end repeats the last row)
#pragma unroll
            for (int u = 0; u < RO_DEPTH; ++u) {
                const bool live = r + u < cnt;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    const double t = spmm::accumulate(acc[v], 1.0, (double)xv[u][v]);
                    acc[v] = live ? t : acc[v];
                }
            }
        }
        ro_emit<T, VEC>(a, l, g, k, n, f0, acc, y);
    }
}

// rows that take P = 2^lg <= 32 lanes: a wave takes 64 / P consecutive chunks of a layer, staged through LDS piece by piece
template <class T, int VEC>
__global__ __launch_bounds__(RO_THREADS, 4) void k_ro_narrow(Ro a, const T* __restrict__ x, T* __restrict__ y) {
    __shared__ __attribute__((aligned(16))) unsigned char tiles[RO_WAVES][RO_TILE_BYTES];
    __shared__ int64_t sh_row[RO_WAVES][64];
    __shared__ int32_t sh_cnt[RO_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int P = 1 << a.lg, C = 64 >> a.lg;
    const int c = lane >> a.lg, j = lane & (P - 1);
    const int64_t f0 = (int64_t)j * VEC;
    const bool col = f0 < a.F;
    const int64_t total = a.choff[a.G];
    const int64_t qgroups = (total + C - 1) / C;
    const int64_t items = a.L * qgroups;
    T* tile = reinterpret_cast<T*>(tiles[wave]);
    const uint32_t F = (uint32_t)a.F;                       // (at most 32 lanes x VEC columns)
    const uint32_t upp = (uint32_t)RO_R * F / VEC;          // units (VEC elements) of a full piece
    const uint32_t stride = (uint32_t)RO_R * F + VEC;       // elements between the pieces of two chunks
    const uint32_t lane_c = (uint32_t)lane / upp, lane_u = (uint32_t)lane % upp, step_c = 64u / upp, step_u = 64u % upp;
#pragma unroll 1
    for (int64_t base = (int64_t)blockIdx.x * RO_WAVES; base < items; base += (int64_t)gridDim.x * RO_WAVES) {   // (the same turns for every wave of the workgroup)
        const int64_t w = base + wave;
        int64_t l = 0, g = 0, k = 0, s = 0, n = 0, row0 = 0;
        int32_t cnt = 0;
        if (w < items) {
            l = w / qgroups;
            const int64_t q = (w - l * qgroups) * C + c;
            if (readout::item_of(a.choff, a.G, q, &g, &k)) {
                readout::graph_range(a.np, g, a.N, &s, &n);
                row0 = s + spmm::chunk_begin(k);
                cnt = (int32_t)readout::clampi(spmm::chunk_end(n, k) - spmm::chunk_begin(k), 0, spmm::CHUNK);
            }
        }
        if (j == 0) { sh_row[wave][c] = row0; sh_cnt[wave][c] = cnt; }
        const T* __restrict__ xl = x + l * a.N * a.F;
        double acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
        // (the barrier that asks whether any lane of the workgroup has rows left also orders the pieces: written, read, written again)
#pragma unroll 1
        for (int32_t t0 = 0; __syncthreads_or(t0 < cnt); t0 += RO_R) {
            T buf[RO_R][VEC];
            const T* src[RO_R];
            uint32_t dst[RO_R];
            bool ok[RO_R];
            uint32_t c2 = lane_c, u = lane_u;   // unit lane + 64 it of the wave's pieces: unit u of chunk c2
#pragma unroll
            for (int it = 0; it < RO_R; ++it, c2 += step_c, u += step_u) {   // C chunks x upp units <= 64 x RO_R: every unit has a turn
                if (u >= upp) { u -= upp; ++c2; }
                const uint32_t cc = c2 < (uint32_t)C ? c2 : 0u;
                const int32_t left = sh_cnt[wave][cc] - t0;
                const uint32_t rows = (uint32_t)(left < 0 ? 0 : (left > RO_R ? RO_R : left));
                ok[it] = c2 < (uint32_t)C && u * VEC < rows * F;
                dst[it] = cc * stride + u * VEC;
                src[it] = ok[it] ? xl + (sh_row[wave][cc] + t0) * a.F + u * VEC : x;   // (a unit without a turn reads the first one of x: no branch between the loads)
            }
#pragma unroll
            for (int it = 0; it < RO_R; ++it) ro_load<T, VEC>(src[it], buf[it]);
#pragma unroll
            for (int it = 0; it < RO_R; ++it) {
                if (ok[it]) ro_store<T, VEC>(tile + dst[it], buf[it]);
            }
            __syncthreads();
            if (col) {
                const int32_t rows = cnt - t0 < RO_R ? cnt - t0 : RO_R;
                const T* tr = tile + (uint32_t)c * stride + (uint32_t)f0;
#pragma unroll
                for (int r = 0; r < RO_R; ++r) {   // (a row past the end is read where it lies in the piece and left out by a select)
                    T xv[VEC];
                    ro_load<T, VEC>(tr + (uint32_t)r * F, xv);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const double t = spmm::accumulate(acc[v], 1.0, (double)xv[v]);
                        acc[v] = r < rows ? t : acc[v];
                    }
                }
            }
        }
        if (col && cnt > 0) ro_emit<T, VEC>(a, l, g, k, n, f0, acc, y);
    }
}

// what the chunk kernels leave: the empty graphs and the graphs longer than one chunk
template <class T>
__global__ __launch_bounds__(RO_THREADS) void k_ro_finish(Ro a, T* __restrict__ y) {
    const int64_t elems = a.L * a.G * a.F;
    for (int64_t e = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x; e < elems; e += (int64_t)gridDim.x * RO_THREADS) {
        const int64_t lg_ = e / a.F, f = e - lg_ * a.F;
        const int64_t l = lg_ / a.G, g = lg_ - l * a.G;
        int64_t s, n;
        readout::graph_range(a.np, g, a.N, &s, &n);
        if (n > 0 && n <= spmm::CHUNK) continue;
        double total = 0.0;
        if (n > spmm::CHUNK) {
            const int64_t nc = spmm::num_chunks(n), p0 = a.poff[g];
            if (p0 >= 0 && p0 + nc <= a.pcap) {   // (else only a table that is not well formed: 0)
                const double* __restrict__ ps = a.part + (l * a.pcap + p0) * a.F + f;
                for (int64_t k = 0; k < nc; k += RO_DEPTH) {   // (the adds are a chain by the rule; the loads of eight chunk sums are not)
                    double v[RO_DEPTH];
#pragma unroll
                    for (int u = 0; u < RO_DEPTH; ++u) v[u] = ps[(k + u < nc ? k + u : nc - 1) * a.F];
#pragma unroll
                    for (int u = 0; u < RO_DEPTH; ++u) total = k + u < nc ? total + v[u] : total;
                }
            }
        }
        y[e] = (T)readout::finish(total, n, a.mean != 0);
    }
}

// gx[l, i, :] = gy[l, g(i), :], for the mean divided by the graph's count
template <class T, int VEC>
__global__ __launch_bounds__(RO_THREADS) void k_ro_backward(Ro a, const T* __restrict__ gy, T* __restrict__ gx) {
    const int64_t upr = a.F / VEC;   // units of a row
    const int64_t tasks = a.N * upr;
    for (int64_t t = (int64_t)blockIdx.x * RO_THREADS + threadIdx.x; t < tasks; t += (int64_t)gridDim.x * RO_THREADS) {
        const int64_t i = t / upr, f0 = (t - i * upr) * VEC;
        const int64_t g = seg_of(a.np, a.G, i);   // (in [0, G) whatever the table holds)
        int64_t s, n;
        readout::graph_range(a.np, g, a.N, &s, &n);
        const bool div = a.mean != 0 && n > 0;
        for (int64_t l = 0; l < a.L; ++l) {
            T v[VEC];
            ro_load<T, VEC>(gy + (l * a.G + g) * a.F + f0, v);
            if (div) {
#pragma unroll
                for (int u = 0; u < VEC; ++u) v[u] = (T)((double)v[u] / (double)n);
            }
            ro_store<T, VEC>(gx + (l * a.N + i) * a.F + f0, v);
        }
    }
}

struct Bufs {
    int32_t *nch, *lch;
    int64_t *choff, *poff;
    void* scan_tmp; size_t scan_bytes;
    double* part; int64_t pcap;
};

size_t carve_readout(Carve& C, int64_t L, int64_t N, int64_t F, int64_t G, Bufs& B) {
    B.nch = C.take<int32_t>(G + 1);
    B.lch = C.take<int32_t>(G + 1);
    B.choff = C.take<int64_t>(G + 1);
    B.poff = C.take<int64_t>(G + 1);
    B.scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, B.scan_bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(G + 1),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    B.scan_tmp = C.take<char>((int64_t)B.scan_bytes);
    B.pcap = readout::part_bound(N, G);
    B.part = C.take<double>(L * B.pcap * F);
    return C.off + 256;
}

// lanes of a row: 16 bytes a lane when F and the pointers allow (readout::dispatch, rlap_readout.h)
template <class T>
readout::Dispatch dispatch_of(int64_t F, const void* p, const void* q) {
    return readout::dispatch(F, (int)sizeof(T), ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q)) & 15) == 0);
}

template <class T>
int launch_readout(hipStream_t st, Ro a, const ReadoutArgs& g) {
    constexpr int V = 16 / (int)sizeof(T);
    const T* x = static_cast<const T*>(g.x);
    T* y = static_cast<T*>(g.y);
    const readout::Dispatch d = dispatch_of<T>(a.F, x, y);
    const bool vec = d.vec;
    a.lg = d.lg;
    a.ftiles = d.ftiles;
    const int64_t bound = readout::chunk_bound(a.N, a.G);
    if (a.N > 0) {
        if (a.lg == 6) {
            const unsigned nb = ro_blocks(a.L * bound * a.ftiles, RO_WAVES);
            if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_wide<T, V>), dim3(nb), dim3(RO_THREADS), 0, st, a, x, y);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_wide<T, 1>), dim3(nb), dim3(RO_THREADS), 0, st, a, x, y);
        } else {
            const int64_t C = 64 >> a.lg;
            const unsigned nb = ro_blocks(a.L * ((bound + C - 1) / C), RO_WAVES);
            if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_narrow<T, V>), dim3(nb), dim3(RO_THREADS), 0, st, a, x, y);
            else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_narrow<T, 1>), dim3(nb), dim3(RO_THREADS), 0, st, a, x, y);
        }
    }
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_finish<T>), dim3(ro_blocks(a.L * a.G * a.F, RO_THREADS)), dim3(RO_THREADS), 0, st, a, y);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

template <class T>
int launch_backward(hipStream_t st, Ro a, const ReadoutArgs& g) {
    constexpr int V = 16 / (int)sizeof(T);
    const T* gy = static_cast<const T*>(g.x);
    T* gx = static_cast<T*>(g.y);
    const readout::Dispatch d = dispatch_of<T>(a.F, gy, gx);
    const bool vec = d.vec;
    const unsigned nb = ro_blocks(a.N * d.lanes, RO_THREADS);
    if (vec) hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_backward<T, V>), dim3(nb), dim3(RO_THREADS), 0, st, a, gy, gx);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(k_ro_backward<T, 1>), dim3(nb), dim3(RO_THREADS), 0, st, a, gy, gx);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace

size_t readout_bytes(int64_t L, int64_t N, int64_t F, int64_t G) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_readout(C, L, N, F, G, B);
}

int readout_run(hipStream_t st, void* ws, size_t ws_bytes, const ReadoutArgs& g) {
    if (g.L == 0) return RLAP_OK;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_readout(C, g.L, g.N, g.F, g.G, B) > ws_bytes) return RLAP_E_WORKSPACE;
    Ro a{};
    a.np = g.node_ptr; a.N = g.N; a.G = g.G; a.L = g.L; a.F = g.F;
    a.mean = (g.flags & RLAP_READOUT_MEAN) ? 1 : 0;
    a.nch = B.nch; a.lch = B.lch; a.choff = B.choff; a.poff = B.poff; a.part = B.part; a.pcap = B.pcap;
    hipLaunchKernelGGL(k_ro_counts, dim3(ro_blocks(g.G + 1, 256)), dim3(256), 0, st, a);
    RLAP_HIPCHK(hipGetLastError());
    size_t sb = B.scan_bytes;
    RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, sb, B.nch, B.choff, (int64_t)0, (size_t)(g.G + 1), rocprim::plus<int64_t>(), st));
    sb = B.scan_bytes;
    RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, sb, B.lch, B.poff, (int64_t)0, (size_t)(g.G + 1), rocprim::plus<int64_t>(), st));
    return (g.flags & RLAP_READOUT_X_F32) ? launch_readout<float>(st, a, g) : launch_readout<double>(st, a, g);
}

int readout_backward_run(hipStream_t st, const ReadoutArgs& g) {
    if (g.L == 0 || g.N == 0) return RLAP_OK;
    Ro a{};
    a.np = g.node_ptr; a.N = g.N; a.G = g.G; a.L = g.L; a.F = g.F;
    a.mean = (g.flags & RLAP_READOUT_MEAN) ? 1 : 0;
    return (g.flags & RLAP_READOUT_X_F32) ? launch_backward<float>(st, a, g) : launch_backward<double>(st, a, g);
}

}  // namespace rlap
