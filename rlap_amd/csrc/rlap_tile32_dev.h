// rlap_tile32_dev.h -- the kernel steps that the streamed-tile kernels share (k_in_main of rlap_infonce.hip, k_g2l_main of
// rlap_g2l.hip), and what rlap_cca.hip takes of them (f32x16, allow_lds, the ladder).  HIP only; the layout they rely on is
// rlap_tile32.h's.  Every function is inlined into its kernel, and the order of its loops is the order of the rule headers' sums:
// the order is the bits.
#pragma once
#include <type_traits>

#include <hip/hip_runtime.h>

#include "rlap_snapshot.h"
#include "rlap_spmm.h"
#include "rlap_tile32.h"

namespace rlap {
namespace tile32 {

typedef float f32x16 __attribute__((ext_vector_type(16)));   // a 32x32 accumulator tile: register r of a lane holds row reg_row(r, lane >> 5)

// X[stream row][owner row] of one tile pair: the chain over the padded columns in increasing k from +0, four MFMAs per 16 bytes of
// either operand's fragment image (nqq = Fp / 8)
__device__ __forceinline__ f32x16 pair_chain(const float4* __restrict__ stream_lds, const float4* __restrict__ owner, int nqq, int lane) {
    f32x16 x;
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = 0.0f;
    for (int qq = 0; qq < nqq; ++qq) {
        const float4 s = stream_lds[qq * 64 + lane];
        const float4 o = owner[qq * 64 + lane];
        x = __builtin_amdgcn_mfma_f32_32x32x2f32(s.x, o.x, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x2f32(s.y, o.y, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x2f32(s.z, o.z, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f32_32x32x2f32(s.w, o.w, x, 0, 0, 0);
    }
    return x;
}

// A workgroup of THREADS stages a stream tile into LDS: its fragment image `frag` and, behind it (rows != nullptr), its row-major
// image `rows` -- the 32 rows of a tile are contiguous there too.  tile_vec = 32 Fp / 4 float4s each.  The caller's barriers stand
// around it.
template <int THREADS>
__device__ __forceinline__ void stage_tile(float* lds, const float* frag, const float* rows, int tile_vec) {
    const float4* __restrict__ src = reinterpret_cast<const float4*>(frag);
    float4* dst = reinterpret_cast<float4*>(lds);
    for (int v = threadIdx.x; v < tile_vec; v += THREADS) dst[v] = src[v];
    if (rows) {
        const float4* __restrict__ src2 = reinterpret_cast<const float4*>(rows);
        for (int v = threadIdx.x; v < tile_vec; v += THREADS) dst[tile_vec + v] = src2[v];
    }
}

// the NFT accumulator tiles of a wave, of which the first nft are live
template <int NFT>
__device__ __forceinline__ void zero_tiles(f32x16 (&acc)[NFT]) {
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ft][r] = 0.0f;
}

// acc[ft] += x^T B: x is the A operand as it stands (register r of the two lane halves is the k pair of step r: stream rows
// reg_row(r, 0), reg_row(r, 1)), B the staged tile's row-major image `rows_lds` (32 x Fp), 32 columns per feature tile.  ft outside,
// r inside.
template <int NFT>
__device__ __forceinline__ void accumulate_tiles(f32x16 (&acc)[NFT], int nft, const f32x16& x, const float* rows_lds, int Fp, int c, int h) {
    const float* brow = rows_lds + 4 * h * Fp + c;   // row reg_row(r, h) = reg_row(r, 0) + 4 h of the staged tile
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) {
        if (ft < nft) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float bv = brow[reg_row(r, 0) * Fp + ft * TILE];
                acc[ft] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[r], bv, acc[ft], 0, 0, 0);
            }
        }
    }
}

// the live tiles to a padded row-major slice: `tile` points at the owner tile's first row, row stride Fp
template <int NFT>
__device__ __forceinline__ void store_tiles(const f32x16 (&acc)[NFT], int nft, float* tile, int Fp, int c, int h) {
    float* __restrict__ out = tile + c;
#pragma unroll
    for (int ft = 0; ft < NFT; ++ft) {
        if (ft < nft) {
#pragma unroll
            for (int r = 0; r < 16; ++r) out[(int64_t)reg_row(r, h) * Fp + ft * TILE] = acc[ft][r];
        }
    }
}

// the chunk sums of `lists` lists of N doubles each (rlap_spmm.h's rule), list l at rows + l N, into csum + l num_chunks(N); the
// body of a striding kernel
__device__ __forceinline__ void chunk_sums(const double* __restrict__ rows, int64_t N, int lists, double* __restrict__ csum) {
    const int64_t nc = spmm::num_chunks(N);
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nc * lists; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t l = q / nc, k = q - l * nc;
        const double* list = rows + l * N;
        csum[q] = spmm::chunk_sum(N, k, [](int64_t) { return 1.0; }, [&](int64_t e) { return list[e]; });
    }
}

// A launch takes up to 48 KB of dynamic LDS unasked; only a larger one raises the function's limit first.  Stateless: nothing is
// remembered per process, so it holds for every device.
template <class K>
int allow_lds(K* fn, size_t lds) {
    if (lds <= 48 * 1024) return RLAP_OK;
    RLAP_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return RLAP_OK;
}

// launch(std::integral_constant<int, I>) for the ladder's instance I of nft; no instance (F outside [1, MAX_F], which the entry
// points refuse) is an error
template <class Launch>
int ladder_launch(int nft, Launch launch) {
    switch (ladder_instance(nft)) {   // the rule is rlap_tile32.h's
        case 1: return launch(std::integral_constant<int, 1>{});
        case 2: return launch(std::integral_constant<int, 2>{});
        case 4: return launch(std::integral_constant<int, 4>{});
        case 8: return launch(std::integral_constant<int, 8>{});
        case 16: return launch(std::integral_constant<int, 16>{});
    }
    return RLAP_E_INTERNAL;
}

}  // namespace tile32
}  // namespace rlap
