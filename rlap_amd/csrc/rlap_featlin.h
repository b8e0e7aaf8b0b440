// rlap_featlin.h -- the sparse first layer (rlap_feature_plan_build / rlap_feature_plan_apply): the rules of a feature
// plan as plain __host__ __device__ functions without any HIP dependency.  tests/csrc/featlin_mirror.cc compiles them with g++ and
// builds and applies a whole plan on the host; the kernels of rlap_featlin.hip read the same functions.
//
// A feature plan holds a dense (N, Fin) matrix x as lists, once per direction:
//   an entry (i, j) is kept iff (double)x[i][j] != 0.0 (-0.0 is dropped; NaN and infinities stay); its coefficient is that double;
//   forward list of row i       : its kept entries by ascending j, records {c, j};
//   transposed list of column j : its kept entries by ascending i, records {c, i}.
// With keep[k][j] != 0 meaning that view k keeps column j:
//   y[k][i][f] : the forward list of i cut into chunks of spmm::CHUNK by position in the FULL list; a chunk is summed from 0.0 in
//                list order by spmm::accumulate(acc, c_e, W[col_e][f]), an entry whose column the view drops leaving acc as it is;
//                the chunk sums are added to 0.0 in chunk order; rounded once to W's type.  Nothing kept: exactly +0.0.
//   dW[j][f]   : for k ascending, if keep[k][j], s_k = spmm::list_sum(list of j, c_e, G[k][row_e][f], no loop); the total is 0.0 +
//                s_k over those views in view order, rounded once.  No view keeps j: exactly +0.0.
// The buffer has, per direction, an int64 offset table ([N + 1] forward, [Fin + 1] transposed), a directory of the chunks of the
// lists longer than CHUNK (in slot order, capacity plan::dir_cap(nnz)) and Record[nnz]; every part is 256-byte aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rlap_plan.h"
#include "rlap_spmm.h"

namespace rlap {
namespace featlin {

constexpr int32_t MAGIC = 0x46454154;    // rlap_feature_desc.magic of a successful build
constexpr int MAX_VIEWS = 32;            // K of a call: the views' keep bits of a column share one 32-bit word
constexpr int VIEW_GROUP = 8;            // views the forward kernel accumulates side by side
constexpr int64_t MAX_DIM = (int64_t)1 << 31;   // N, Fin below it (record ids are int32)
constexpr int64_t MAX_NNZ = ((int64_t)1 << 31) - 1;

// whether an entry is in the lists
RLAP_SPMM_HD bool kept(double v) { return v != 0.0; }

// byte offsets of the parts of a feature plan buffer (-1: the part is not there): offsets, directories, records, each forward
// first, so that the records are the buffer's tail
struct Layout {
    int64_t off[2];               // int64[N + 1] forward, int64[Fin + 1] transposed
    int64_t dir[2];               // ChunkRef[dir_cap(nnz)]
    int64_t rec[2];               // Record[nnz]
    int64_t bytes;
};
RLAP_SPMM_HD Layout layout(int64_t N, int64_t Fin, int64_t nnz, bool forward, bool transposed) {
    Layout L;
    int64_t at = 0;
    const bool has[2] = {forward, transposed};
    const int64_t slots[2] = {N, Fin};
    for (int d = 0; d < 2; ++d) {
        L.off[d] = -1;
        if (has[d]) { L.off[d] = at; at = plan::align_up(at + 8 * (slots[d] + 1)); }
    }
    for (int d = 0; d < 2; ++d) {
        L.dir[d] = -1;
        if (has[d]) { L.dir[d] = at; at = plan::align_up(at + (int64_t)sizeof(plan::ChunkRef) * plan::dir_cap(nnz)); }
    }
    for (int d = 0; d < 2; ++d) {
        L.rec[d] = -1;
        if (has[d]) { L.rec[d] = at; at = plan::align_up(at + (int64_t)sizeof(plan::Record) * nnz); }
    }
    L.bytes = at > 0 ? at : 256;
    return L;
}

// whether the parts of one direction -- `slots` lists, `entries` records, `chunks` directory entries at the byte offsets off / dir /
// rec -- lie inside a buffer of `bytes` bytes, 16-byte aligned: what a planned call checks before it reads anything
RLAP_SPMM_HD bool parts_inside(int64_t slots, int64_t entries, int64_t chunks, int64_t off, int64_t dir, int64_t rec, int64_t nnz, int64_t bytes) {
    if (slots < 1 || entries < 0 || entries > nnz || chunks < 0 || chunks > plan::dir_cap(nnz)) return false;
    if (off < 0 || dir < 0 || rec < 0 || ((off | dir | rec) & 15)) return false;
    return off + 8 * (slots + 1) <= bytes && dir + 16 * chunks <= bytes && rec + 16 * entries <= bytes;
}

RLAP_SPMM_HD int64_t clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the sum of chunk k of a forward list under one view's mask: coef(e), feat(e) as in rlap_spmm.h, col_kept(e) whether the view
// keeps entry e's column
template <class Coef, class Feat, class ColKept>
RLAP_SPMM_HD double masked_chunk_sum(int64_t n, int64_t k, Coef coef, Feat feat, ColKept col_kept) {
    double s = 0.0;
    for (int64_t e = spmm::chunk_begin(k); e < spmm::chunk_end(n, k); ++e)
        if (col_kept(e)) s = spmm::accumulate(s, coef(e), feat(e));
    return s;
}

// y[k][i][f] before it is rounded: the forward list's n entries
template <class Coef, class Feat, class ColKept>
RLAP_SPMM_HD double forward_value(int64_t n, Coef coef, Feat feat, ColKept col_kept) {
    double total = 0.0;
    for (int64_t k = 0; k < spmm::num_chunks(n); ++k) total = total + masked_chunk_sum(n, k, coef, feat, col_kept);
    return total;
}

// dW[j][f] before it is rounded: view_kept(k) says whether view k keeps j, view_sum(k) is s_k
template <class ViewKept, class ViewSum>
RLAP_SPMM_HD double transposed_value(int K, ViewKept view_kept, ViewSum view_sum) {
    double total = 0.0;
    for (int k = 0; k < K; ++k)
        if (view_kept(k)) total = total + view_sum(k);
    return total;
}

}  // namespace featlin
}  // namespace rlap
