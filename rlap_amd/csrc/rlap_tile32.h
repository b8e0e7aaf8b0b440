// rlap_tile32.h -- the 32x32 tile that the fused losses and the probe are cut into (rlap_infonce.h, rlap_g2l.h, rlap_cca.h,
// rlap_probe.h), written down once: the tile counts and padded sizes, the register layout of an accumulator tile, the fragment
// image and the instance ladder.  Plain __host__ __device__ functions without any HIP dependency, as rlap_spmm.h: the mirrors under
// tests/csrc compile this file with g++, the kernels read the same functions.  The rule headers import these names with
// using-declarations, so infonce::reg_row, cca::padded_rows and the like are these functions.
//
// The register layout.  v_mfma_f32_32x32x2_f32 leaves a 32x32 accumulator tile in 16 registers of 64 lanes: the tile's column is
// lane & 31, and register r of a lane of half h = lane >> 5 holds row reg_row(r, h) = (r & 3) + 8 (r >> 2) + 4 h -- rows
// 0 1 2 3 8 9 10 11 ... in half 0 and the same + 4 in half 1.  Fed to the next 32x32x2 MFMA as its A operand as it stands,
// register r of the two halves is the k pair of step r, so the rows enter a chain in the order 0 4 1 5 2 6 3 7 8 12 ...: r
// outside, h inside.  Every rule that sums over the rows of a tile names this order.
//
// The fragment image.  An operand of one 32x32x2 MFMA is one float a lane: lane = 32 (k & 1) + row for the k pair (2 q, 2 q + 1).
// The image stores a 32-row tile as one contiguous block, eight columns (four k pairs) by eight columns, 64 lanes x 4 floats: the
// 16 bytes of a lane are its operands of four consecutive MFMAs, and a wave reads 1 KiB an instruction (frag_offset).
#pragma once
#include <stdint.h>

#include "rlap_spmm.h"

namespace rlap {
namespace tile32 {

constexpr int TILE = 32;                  // rows and columns of a tile (one 32x32 MFMA accumulator)
constexpr int BLOCK_TILES = 4;            // owner tiles of a workgroup of the streamed-tile kernels (one per wave)
constexpr int MAX_INSTANCE = 16;          // the largest instance of the ladder: 16 tiles of 32 columns, 512 feature columns

// the 32-row tiles of n rows, the workgroups' row blocks, the padded sizes of the arenas' copies, the 32-column tiles of F columns
RLAP_SPMM_HD int64_t num_tiles(int64_t n) { return n > 0 ? (n + TILE - 1) / TILE : 0; }
RLAP_SPMM_HD int64_t row_blocks(int64_t n) { return (num_tiles(n) + BLOCK_TILES - 1) / BLOCK_TILES; }
RLAP_SPMM_HD int64_t padded_rows(int64_t n) { return num_tiles(n) * TILE; }
RLAP_SPMM_HD int feature_tiles(int64_t F) { return (int)((F + TILE - 1) / TILE); }
RLAP_SPMM_HD int padded_features(int64_t F) { return feature_tiles(F) * TILE; }

// row of a 32x32 accumulator tile that register r of a lane of half h holds (the tile's column is lane & 31)
RLAP_SPMM_HD int reg_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// where element (row i, column k) of a padded copy lies in its fragment image (Fp: the padded columns)
RLAP_SPMM_HD int64_t frag_offset(int64_t i, int k, int Fp) {
    const int64_t t = i >> 5;
    const int r = (int)(i & 31), q = k >> 1;
    return ((t * (Fp >> 3) + (q >> 2)) * 64 + (k & 1) * 32 + r) * 4 + (q & 3);
}

// The instance ladder: a kernel template that holds NFT tiles (or stages NV float4s) a wave and guards each with ft < nft is
// instantiated for 1, 2, 4, 8, 16; a call of nft = feature_tiles(F) takes the smallest that holds nft.  0 for an nft outside
// [1, MAX_INSTANCE], which no launcher accepts.
RLAP_SPMM_HD int ladder_instance(int nft) {
    if (nft < 1 || nft > MAX_INSTANCE) return 0;
    return nft <= 1 ? 1 : (nft <= 2 ? 2 : (nft <= 4 ? 4 : (nft <= 8 ? 8 : 16)));
}

}  // namespace tile32
}  // namespace rlap
