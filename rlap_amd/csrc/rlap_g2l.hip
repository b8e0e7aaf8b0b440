// rlap_g2l.hip -- the fused graph-to-local losses, forward and backward (rlap_g2l_jsd / rlap_g2l_bootstrap and their backward calls,
// DESIGN 4.17): one direction of DualBranchContrast(JSD(), mode="G2L") and of BootstrapContrast(BootstrapLatent(), mode="G2L")
// without the concatenated (2N, F) copy, the dense (G, N) masks and the dense similarity matrix.  Every value and the order of every
// sum are rlap_g2l.h's.  A translation unit of its own.
//
//   pre-pass   the node -> graph map from node_ptr (every value read from the table is clamped before it is compared: the map lies
//              in [0, G) whatever the table holds; the table is never read back).  JSD, G >= 2: the zero-padded images of h and g,
//              the FRAGMENT image of rlap_tile32.h and (backward) the row-major image.  Bootstrap: the hat image of g.
//   JSD main   G >= 2: rlap_infonce.hip's structure with a short stream.  A workgroup of four waves OWNS four 32-row tiles of one
//              input and walks the 32-row tiles of the other, staged through LDS once for the four waves; per tile a wave computes
//              X[stream row][owner row] with v_mfma_f32_32x32x2_f32.
//                forward   the nodes own, the graphs stream: the terms are added in register order into the lane's float64 sum,
//                          the positive pair is kept apart, padding graphs and the positive are left out of the sum.
//                dh        the same, the weights replace the scores in their registers and are the A operand of the second
//                          product with the graphs' row-major image in LDS; the accumulators are dh.
//                dg        the graphs own, the nodes stream over the workgroup's PART of the node tiles; the accumulators go to
//                          the part's slice, and a finish kernel adds the slices in part order.
//   vector     G == 1 and the bootstrap need one dot product per node with one vector: a memory-bound pass.  A block stages its
//              rows in LDS with coalesced 16-byte loads (an odd row stride: no bank conflicts), then one thread per row walks its
//              row in k order -- the same fmaf chain as the matrix core's.  Every row is read once.
//   finish     the chunk-rule sums; one thread writes the loss.
// No float atomics, no host synchronisation, nothing allocated outside the arena.
#include <algorithm>

#include <hip/hip_runtime.h>

#include "../../include/rlap_hip.h"
#include "rlap_g2l.h"
#include "rlap_g2l_api.h"
#include "rlap_spmm.h"
#include "rlap_tile32_dev.h"

namespace rlap {
namespace {

using tile32::f32x16;

constexpr int GL_THREADS = 256;                 // four waves: g2l::BLOCK_TILES owner tiles
constexpr int64_t GL_MAX_GRID = 1 << 20;        // workgroups of a striding launch
static_assert(GL_THREADS == 64 * g2l::BLOCK_TILES, "one wave per owner tile");
static_assert(GL_THREADS == g2l::VEC_THREADS, "one thread per staged row");

inline unsigned gl_blocks(int64_t n, int per_block) { return capped_blocks(n, per_block, GL_MAX_GRID); }

// ------------------------------------------------------------------------------------------------ pre-pass
// map[i] = g(i) for i < N, 0 behind (`len` entries)
__global__ __launch_bounds__(256) void k_g2l_map(const int64_t* __restrict__ node_ptr, int64_t G, int64_t N, int64_t len, int32_t* __restrict__ map) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x)
        map[i] = i < N ? (int32_t)g2l::graph_of(node_ptr, G, N, i) : 0;
}

// the copy of x padded with zeros: the fragment image and (rows != nullptr) the row-major image
__global__ __launch_bounds__(256) void k_g2l_pad(const float* __restrict__ x, int64_t N, int64_t F, int64_t Np, int Fp, float* __restrict__ frag,
                                                 float* __restrict__ rows) {
    const int64_t elems = Np * Fp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < elems; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / Fp;
        const int k = (int)(e - i * Fp);
        const float v = (i < N && k < F) ? x[i * F + k] : 0.0f;
        frag[tile32::frag_offset(i, k, Fp)] = v;
        if (rows) rows[e] = v;
    }
}

// the hat image of g (the norm stays in a register), one thread per graph
__global__ __launch_bounds__(256) void k_g2l_ghat(const float* __restrict__ g, int64_t G, int64_t F, float* __restrict__ ghat) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < G; j += (int64_t)gridDim.x * blockDim.x) {
        const double nrm = infonce::norm_of(infonce::norm2(g + j * F, F));
        for (int64_t k = 0; k < F; ++k) ghat[j * F + k] = infonce::hat(g[j * F + k], nrm);
    }
}

// ------------------------------------------------------------------------------------------------ JSD main, G >= 2
struct Main {
    const float* own_frag; const float* str_frag;   // fragment images, padded rows x Fp each
    const float* str_rows;                          // backward: the stream's row-major image
    const int32_t* map;                             // [Np] g(i), 0 behind N
    const double* gup;                              // backward: the upstream gradient
    int64_t N, G, F; int64_t To, Ts, RB; int parts; int Fp; int nft;
    double* rows;                                   // forward: [2 N] pos_i, neg_i
    float* out;                                     // dh: (N, F)
    float* partial; int64_t Gp;                     // dg: [parts, Gp, Fp] part accumulators
};

enum { GL_FORWARD = 0, GL_BACK_DH = 1, GL_BACK_DG = 2 };

template <int NFT, int MODE>
__global__ __launch_bounds__(GL_THREADS) void k_g2l_main(Main a) {
    extern __shared__ __attribute__((aligned(16))) float gl_lds[];   // 32 x Fp floats: the stream tile's fragment image; backward: and its row-major image
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = lane & 31, hf = lane >> 5;
    const int64_t blk = (int64_t)blockIdx.x % a.RB, part = (int64_t)blockIdx.x / a.RB;
    const int64_t ot = blk * g2l::BLOCK_TILES + wave;
    const bool active = ot < a.To;                                   // (wave-uniform)
    const int64_t tile_floats = (int64_t)g2l::TILE * a.Fp;
    const int tile_vec = (int)(tile_floats >> 2), nqq = a.Fp >> 3;
    const float4* __restrict__ owner = reinterpret_cast<const float4*>(a.own_frag + (active ? ot : 0) * tile_floats);
    const int64_t orow = ot * g2l::TILE + c;                         // the lane's owner row (inside the padded rows when active)
    const int64_t tb = MODE == GL_BACK_DG ? g2l::part_begin(a.N, a.G, a.F, part) : 0;
    const int64_t te = MODE == GL_BACK_DG ? g2l::part_begin(a.N, a.G, a.F, part + 1) : a.Ts;

    int64_t gi_lane = 0;                                             // nodes own: the lane's graph
    if (MODE != GL_BACK_DG && active) gi_lane = a.map[orow];
    double cp = 0.0, cn = 0.0;
    if (MODE != GL_FORWARD) {
        const double gup = *a.gup;
        cp = g2l::pos_coef(gup, a.N);
        cn = g2l::neg_coef(gup, a.N, a.G);
    }
    double nsum = 0.0, pos = 0.0;
    int have = 0;
    f32x16 acc[NFT];
    if (MODE != GL_FORWARD) tile32::zero_tiles(acc);

#pragma unroll 1
    for (int64_t t = tb; t < te; ++t) {
        __syncthreads();   // (the previous tile has been read)
        tile32::stage_tile<GL_THREADS>(gl_lds, a.str_frag + t * tile_floats, MODE != GL_FORWARD ? a.str_rows + t * tile_floats : nullptr, tile_vec);
        __syncthreads();
        if (!active) continue;
        f32x16 x = tile32::pair_chain(reinterpret_cast<const float4*>(gl_lds), owner, nqq, lane);
        const int64_t srow0 = t * g2l::TILE;
        if (MODE == GL_FORWARD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t j = srow0 + g2l::reg_row(r, hf);       // the graph
                double pt, nt;
                g2l::terms(x[r], &pt, &nt);
                const double n2 = nsum + nt;
                const bool mine = j == gi_lane;
                nsum = (j < a.G && !mine) ? n2 : nsum;
                pos = mine ? pt : pos;
                have = mine ? 1 : have;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t srow = srow0 + g2l::reg_row(r, hf);
                int64_t node, graph, gi;
                if (MODE == GL_BACK_DH) { node = orow; graph = srow; gi = gi_lane; }
                else { node = srow; graph = orow; gi = a.map[srow]; }   // (srow inside the padded nodes)
                const float w = g2l::weight(cp, cn, x[r], graph == gi);
                x[r] = (node < a.N && graph < a.G) ? w : 0.0f;
            }
            tile32::accumulate_tiles(acc, a.nft, x, gl_lds + (int)tile_floats, a.Fp, c, hf);
        }
    }

    if (!active) return;
    if (MODE == GL_FORWARD) {
        const double other_n = __shfl_xor(nsum, 32);
        const double other_p = __shfl_xor(pos, 32);
        if (hf == 0 && orow < a.N) {
            a.rows[orow] = have ? pos : other_p;                     // (exactly one half met the positive)
            a.rows[a.N + orow] = nsum + other_n;                     // half 0 + half 1
        }
    } else if (MODE == GL_BACK_DH) {
#pragma unroll
        for (int ft = 0; ft < NFT; ++ft) {
            if (ft < a.nft) {
                const int64_t col = ft * g2l::TILE + c;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int64_t row = ot * g2l::TILE + g2l::reg_row(r, hf);
                    if (row < a.N && col < a.F) a.out[row * a.F + col] = acc[ft][r];
                }
            }
        }
    } else {
        tile32::store_tiles(acc, a.nft, a.partial + (part * a.Gp + ot * g2l::TILE) * a.Fp, a.Fp, c, hf);
    }
}

// ------------------------------------------------------------------------------------------------ the vector kernels
struct Vec {
    const float* h; const float* neg; const float* g;   // g: the one graph's summary (JSD)
    const float* ghat; const int32_t* map;              // bootstrap: the hat image of g, g(i)
    const double* gup;
    int64_t N; int F;
    double* rows;                                       // forward
    float* w; float* gh; float* gneg;                   // JSD backward: [2 N] weights; dh, dneg
};

enum { V_JSD_FORWARD = 0, V_JSD_BACKWARD = 1, V_BOOT_FORWARD = 2 };

// `total` floats from src (rows of F, contiguous) into LDS rows of stride Fs: 16-byte loads where src allows them
__device__ inline void gl_stage_rows(const float* __restrict__ src, int total, int F, int Fs, float* lds) {
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0) {   // (block-uniform)
        const int nvec = total >> 2;
        const float4* __restrict__ v = reinterpret_cast<const float4*>(src);
        for (int q = threadIdx.x; q < nvec; q += GL_THREADS) {
            const float4 val = v[q];
            const float vals[4] = {val.x, val.y, val.z, val.w};
            int r = (q << 2) / F, k = (q << 2) - r * F;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                lds[r * Fs + k] = vals[u];
                if (++k == F) { k = 0; ++r; }
            }
        }
        done = nvec << 2;
    }
    for (int e = done + threadIdx.x; e < total; e += GL_THREADS) {
        const int r = e / F, k = e - r * F;
        lds[r * Fs + k] = src[e];
    }
}

template <int MODE>
__global__ __launch_bounds__(GL_THREADS) void k_g2l_vec(Vec a) {
    extern __shared__ __attribute__((aligned(16))) float gl_lds[];   // vec_rows(F) rows of stride vec_stride(F)
    __shared__ float wl[g2l::VEC_THREADS];
    const int R = g2l::vec_rows(a.F), Fs = g2l::vec_stride(a.F), F = a.F;
    const int64_t nblk = g2l::vec_blocks(a.N, a.F);
    const int tid = threadIdx.x;
    double cp = 0.0, cn = 0.0;
    if (MODE == V_JSD_BACKWARD) {
        const double gup = *a.gup;
        cp = g2l::pos_coef(gup, a.N);
        cn = g2l::neg_coef(gup, a.N, 1);
    }
    const int npass = MODE == V_BOOT_FORWARD ? 1 : 2;
    for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const int64_t i0 = blk * R;
        const int nrows = (int)(a.N - i0 < R ? a.N - i0 : R);
        for (int pass = 0; pass < npass; ++pass) {
            __syncthreads();   // (the previous rows have been read)
            gl_stage_rows((pass ? a.neg : a.h) + i0 * F, nrows * F, F, Fs, gl_lds);
            __syncthreads();
            if (tid < nrows) {
                const float* row = gl_lds + tid * Fs;
                const int64_t i = i0 + tid;
                float s = 0.0f;
                if (MODE == V_BOOT_FORWARD) {
                    double n2 = 0.0;
                    for (int k = 0; k < F; ++k) n2 = infonce::norm2_step(n2, row[k]);
                    const double nrm = infonce::norm_of(n2);
                    const float* __restrict__ gv = a.ghat + (int64_t)a.map[i] * F;   // (map in [0, G))
                    for (int k = 0; k < F; ++k) s = g2l::score_step(s, gv[k], infonce::hat(row[k], nrm));
                    a.rows[i] = (double)s;
                } else {
                    for (int k = 0; k < F; ++k) s = g2l::score_step(s, a.g[k], row[k]);
                    if (MODE == V_JSD_FORWARD) {
                        a.rows[pass * a.N + i] = pass ? g2l::neg_term(s) : g2l::pos_term(s);
                    } else {
                        const float w = g2l::weight(cp, cn, s, pass == 0);
                        a.w[pass * a.N + i] = w;
                        wl[tid] = w;
                    }
                }
            }
            if (MODE == V_JSD_BACKWARD) {
                __syncthreads();
                float* __restrict__ out = (pass ? a.gneg : a.gh) + i0 * F;
                for (int e = tid; e < nrows * F; e += GL_THREADS) {
                    const int r = e / F, k = e - r * F;
                    out[e] = fmaf(wl[r], a.g[k], 0.0f);
                }
            }
        }
    }
}

// dg of a single graph: the part's nodes in increasing order, one thread per column
__global__ __launch_bounds__(256) void k_g2l_dg_vec(const float* __restrict__ h, const float* __restrict__ neg, const float* __restrict__ w,
                                                    int64_t N, int64_t F, float* __restrict__ partial) {
    const int64_t p = blockIdx.x;
    const int64_t k = (int64_t)blockIdx.y * blockDim.x + threadIdx.x;
    if (k >= F) return;
    const int64_t ib = g2l::part_begin(N, 1, F, p) * g2l::TILE;
    int64_t ie = g2l::part_begin(N, 1, F, p + 1) * g2l::TILE;
    ie = ie < N ? ie : N;
    float acc = 0.0f;
    for (int64_t i = ib; i < ie; ++i) {
        acc = fmaf(w[i], h[i * F + k], acc);
        acc = fmaf(w[N + i], neg[i * F + k], acc);
    }
    partial[p * F + k] = acc;
}

// dg = 0 + part 0 + part 1 + ...; the slices are [parts, rows_p, Fp]
__global__ __launch_bounds__(256) void k_g2l_dg_finish(const float* __restrict__ partial, int64_t parts, int64_t G, int64_t F, int64_t rows_p,
                                                       int64_t Fp, float* __restrict__ dg) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < G * F; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = e / F, k = e - j * F;
        float acc = 0.0f;
        for (int64_t p = 0; p < parts; ++p) acc = acc + partial[(p * rows_p + j) * Fp + k];
        dg[e] = acc;
    }
}

// the bootstrap's gradient: one wave per node, lanes along the columns; the norm and the dot product are the same sequential
// chain on every lane (the LDS reads broadcast), the lanes push their columns through the normalisation in float64
constexpr int GL_GRAD_WAVES = 4;
__global__ __launch_bounds__(64 * GL_GRAD_WAVES) void k_g2l_boot_grad(const float* __restrict__ h, const float* __restrict__ ghat,
                                                                      const int32_t* __restrict__ map, const double* __restrict__ gup, int64_t N,
                                                                      int64_t F, int64_t G, float* __restrict__ out) {
    __shared__ double gh[GL_GRAD_WAVES][g2l::MAX_F];
    __shared__ float oh[GL_GRAD_WAVES][g2l::MAX_F];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double scale = g2l::boot_scale(*gup, G);
    for (int64_t base = (int64_t)blockIdx.x * GL_GRAD_WAVES; base < N; base += (int64_t)gridDim.x * GL_GRAD_WAVES) {   // (the same turns for every wave)
        const int64_t i = base + wave;
        const bool live = i < N;
        if (live)
            for (int k = lane; k < F; k += 64) oh[wave][k] = h[i * F + k];
        __syncthreads();
        double n2 = 0.0;
        if (live)
            for (int k = 0; k < F; ++k) n2 = infonce::norm2_step(n2, oh[wave][k]);
        const double nrm = infonce::norm_of(n2);
        const bool clamped = infonce::norm_clamped(n2);
        __syncthreads();   // (the raw row has been read before its hat image replaces it)
        if (live) {
            const int64_t gi = map[i];   // (in [0, G))
            for (int k = lane; k < F; k += 64) {
                oh[wave][k] = infonce::hat(oh[wave][k], nrm);
                gh[wave][k] = g2l::boot_grad_hat(scale, ghat[gi * F + k]);
            }
        }
        __syncthreads();
        if (live) {
            double dot = 0.0;
            for (int k = 0; k < F; ++k) dot = infonce::dot_step(dot, oh[wave][k], gh[wave][k]);
            for (int k = lane; k < F; k += 64) out[i * F + k] = infonce::grad_in(gh[wave][k], oh[wave][k], dot, nrm, clamped);
        }
        __syncthreads();   // (the row has been read before the next one is written)
    }
}

// ------------------------------------------------------------------------------------------------ finish
// chunk sums of `lists` lists of N doubles each, list l at rows + l N, into csum + l num_chunks(N)
__global__ __launch_bounds__(256) void k_g2l_chunks(const double* __restrict__ rows, int64_t N, int lists, double* __restrict__ csum) {
    tile32::chunk_sums(rows, N, lists, csum);
}

__global__ void k_g2l_loss(const double* __restrict__ csum, int64_t N, int64_t G, int boot, double* __restrict__ loss) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t nc = spmm::num_chunks(N);
    double t0 = 0.0, t1 = 0.0;
    for (int64_t k = 0; k < nc; ++k) t0 = t0 + csum[k];
    if (boot) { *loss = g2l::boot_loss(t0, G); return; }
    for (int64_t k = 0; k < nc; ++k) t1 = t1 + csum[nc + k];
    *loss = g2l::jsd_loss(t0, t1, N, G);
}

// ------------------------------------------------------------------------------------------------ host
template <class T>
T* piece(void* ws, const g2l::Arena& A, int p) {
    return A.off[p] < 0 ? nullptr : reinterpret_cast<T*>(static_cast<char*>(ws) + A.off[p]);
}

template <int NFT, int MODE>
int launch_main_t(hipStream_t st, const Main& m) {
    const size_t lds = (size_t)g2l::TILE * m.Fp * sizeof(float) * (MODE == GL_FORWARD ? 1 : 2);
    if (const int rc = tile32::allow_lds(&k_g2l_main<NFT, MODE>, lds)) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_g2l_main<NFT, MODE>), dim3((unsigned)(m.RB * m.parts)), dim3(GL_THREADS), lds, st, m);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

template <int MODE>
int launch_backward_main(hipStream_t st, const Main& m) {
    return tile32::ladder_launch(m.nft, [&](auto nft) { return launch_main_t<decltype(nft)::value, MODE>(st, m); });
}

template <int MODE>
int launch_vec(hipStream_t st, const Vec& v) {
    const size_t lds = (size_t)g2l::vec_rows(v.F) * g2l::vec_stride(v.F) * sizeof(float);
    if (const int rc = tile32::allow_lds(&k_g2l_vec<MODE>, lds)) return rc;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_g2l_vec<MODE>), dim3(gl_blocks(g2l::vec_blocks(v.N, v.F), 1)), dim3(GL_THREADS), lds, st, v);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int finish_loss(hipStream_t st, const G2lArgs& g, double* csum, int lists) {
    hipLaunchKernelGGL(k_g2l_chunks, dim3(gl_blocks(spmm::num_chunks(g.N) * lists, 256)), dim3(256), 0, st, (const double*)g.rows, g.N, lists, csum);
    hipLaunchKernelGGL(k_g2l_loss, dim3(1), dim3(64), 0, st, (const double*)csum, g.N, g.G, lists == 1 ? 1 : 0, g.loss);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int jsd_many(int call, hipStream_t st, void* ws, const g2l::Arena& A, const G2lArgs& g) {
    const bool back = call == g2l::JSD_BACKWARD;
    const int64_t Np = g2l::padded_rows(g.N), Gp = g2l::padded_rows(g.G);
    const int Fp = g2l::padded_features(g.F);
    int32_t* map = piece<int32_t>(ws, A, g2l::P_MAP);
    float *h_frag = piece<float>(ws, A, g2l::P_HFRAG), *g_frag = piece<float>(ws, A, g2l::P_GFRAG);
    float *h_rows = piece<float>(ws, A, g2l::P_HROWS), *g_rows = piece<float>(ws, A, g2l::P_GROWS);
    hipLaunchKernelGGL(k_g2l_map, dim3(gl_blocks(Np, 256)), dim3(256), 0, st, g.node_ptr, g.G, g.N, Np, map);
    hipLaunchKernelGGL(k_g2l_pad, dim3(gl_blocks(Np * Fp, 256)), dim3(256), 0, st, g.h, g.N, g.F, Np, Fp, h_frag, h_rows);
    hipLaunchKernelGGL(k_g2l_pad, dim3(gl_blocks(Gp * Fp, 256)), dim3(256), 0, st, g.g, g.G, g.F, Gp, Fp, g_frag, g_rows);
    RLAP_HIPCHK(hipGetLastError());
    Main m{};
    m.map = map; m.gup = g.gup; m.N = g.N; m.G = g.G; m.F = g.F; m.Fp = Fp; m.nft = Fp / g2l::TILE; m.Gp = Gp;
    // the nodes own, the graphs stream
    m.own_frag = h_frag; m.str_frag = g_frag; m.str_rows = g_rows;
    m.To = g2l::num_tiles(g.N); m.Ts = g2l::num_tiles(g.G); m.RB = g2l::row_blocks(g.N); m.parts = 1;
    if (!back) {
        m.rows = g.rows;
        if (const int rc = launch_main_t<1, GL_FORWARD>(st, m)) return rc;
        return finish_loss(st, g, piece<double>(ws, A, g2l::P_CSUM), 2);
    }
    m.out = g.gh;
    if (const int rc = launch_backward_main<GL_BACK_DH>(st, m)) return rc;
    // the graphs own, the nodes stream in parts
    float* partial = piece<float>(ws, A, g2l::P_PARTIAL);
    m.own_frag = g_frag; m.str_frag = h_frag; m.str_rows = h_rows; m.partial = partial;
    m.To = g2l::num_tiles(g.G); m.Ts = g2l::num_tiles(g.N); m.RB = g2l::row_blocks(g.G); m.parts = (int)g2l::num_parts(g.N, g.G, g.F);
    if (const int rc = launch_backward_main<GL_BACK_DG>(st, m)) return rc;
    hipLaunchKernelGGL(k_g2l_dg_finish, dim3(gl_blocks(g.G * g.F, 256)), dim3(256), 0, st, (const float*)partial, (int64_t)m.parts, g.G, g.F, Gp,
                       (int64_t)Fp, g.gg);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int jsd_single(int call, hipStream_t st, void* ws, const g2l::Arena& A, const G2lArgs& g) {
    Vec v{};
    v.h = g.h; v.neg = g.neg; v.g = g.g; v.gup = g.gup; v.N = g.N; v.F = (int)g.F;
    if (call == g2l::JSD_FORWARD) {
        v.rows = g.rows;
        if (const int rc = launch_vec<V_JSD_FORWARD>(st, v)) return rc;
        return finish_loss(st, g, piece<double>(ws, A, g2l::P_CSUM), 2);
    }
    float* partial = piece<float>(ws, A, g2l::P_PARTIAL);
    v.w = piece<float>(ws, A, g2l::P_W); v.gh = g.gh; v.gneg = g.gneg;
    if (const int rc = launch_vec<V_JSD_BACKWARD>(st, v)) return rc;
    const int64_t parts = g2l::num_parts(g.N, 1, g.F);
    hipLaunchKernelGGL(k_g2l_dg_vec, dim3((unsigned)parts, (unsigned)((g.F + 255) / 256)), dim3(256), 0, st, g.h, g.neg, (const float*)v.w, g.N, g.F,
                       partial);
    hipLaunchKernelGGL(k_g2l_dg_finish, dim3(gl_blocks(g.F, 256)), dim3(256), 0, st, (const float*)partial, parts, (int64_t)1, g.F, (int64_t)1, g.F,
                       g.gg);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int bootstrap(int call, hipStream_t st, void* ws, const g2l::Arena& A, const G2lArgs& g) {
    int32_t* map = piece<int32_t>(ws, A, g2l::P_MAP);
    float* ghat = piece<float>(ws, A, g2l::P_GHAT);
    hipLaunchKernelGGL(k_g2l_map, dim3(gl_blocks(g.N, 256)), dim3(256), 0, st, g.node_ptr, g.G, g.N, g.N, map);
    hipLaunchKernelGGL(k_g2l_ghat, dim3(gl_blocks(g.G, 256)), dim3(256), 0, st, g.g, g.G, g.F, ghat);
    RLAP_HIPCHK(hipGetLastError());
    if (call == g2l::BOOT_FORWARD) {
        Vec v{};
        v.h = g.h; v.ghat = ghat; v.map = map; v.N = g.N; v.F = (int)g.F; v.rows = g.rows;
        if (const int rc = launch_vec<V_BOOT_FORWARD>(st, v)) return rc;
        return finish_loss(st, g, piece<double>(ws, A, g2l::P_CSUM), 1);
    }
    hipLaunchKernelGGL(k_g2l_boot_grad, dim3(gl_blocks(g.N, GL_GRAD_WAVES)), dim3(64 * GL_GRAD_WAVES), 0, st, g.h, (const float*)ghat,
                       (const int32_t*)map, g.gup, g.N, g.F, g.G, g.gh);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

}  // namespace

size_t g2l_bytes(int call, int64_t N, int64_t G, int64_t F) { return (size_t)g2l::arena(call, N, G, F).bytes; }

int g2l_run(int call, hipStream_t st, void* ws, size_t ws_bytes, const G2lArgs& g) {
    const g2l::Arena A = g2l::arena(call, g.N, g.G, g.F);
    if ((size_t)A.bytes > ws_bytes) return RLAP_E_WORKSPACE;
    if (call == g2l::BOOT_FORWARD || call == g2l::BOOT_BACKWARD) return bootstrap(call, st, ws, A, g);
    return g.G >= 2 ? jsd_many(call, st, ws, A, g) : jsd_single(call, st, ws, A, g);
}

}  // namespace rlap
