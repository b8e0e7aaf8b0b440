// rlap_featlin_api.h -- the sparse first layer (rlap_feature_count / _plan_build / _plan_apply): the interface between
// rlap_featlin.hip, which holds the kernels and their orchestration, and the C ABI in rlap_api.hip, which owns the handle, its lock
// and its arena.  The rules themselves are in rlap_featlin.h.
#pragma once
#include "rlap_featlin.h"
#include "rlap_snapshot.h"

namespace rlap {

struct FeatureBuildArgs {
    const void* x; int64_t N, Fin;            // (N, Fin) row-major; float32 with RLAP_FEAT_X_F32
    int64_t nnz;                              // the caller's count
    int flags;                                // RLAP_FEAT_X_F32, RLAP_PLAN_* resolved
    void* plan; size_t plan_bytes;            // the caller's buffer
};

struct FeatureReport {
    int64_t nnz;
    int64_t longest[2], long_lists[2], chunks[2];   // per direction (-1: not built)
    int32_t host_syncs;
};

struct FeatureApplyArgs {
    const void* plan; const rlap_feature_desc* desc;
    int flags;                                // RLAP_SPMM_TRANSPOSE, RLAP_SPMM_X_F32
    const void* w; const uint8_t* keep; int64_t K, Fout; void* out;
    int64_t part_limit;                       // test hook: directory entries whose chunk sums the call may keep (negative: the budget)
};

// arena bytes of the count, and the count on `stream` (one host synchronisation)
size_t feature_count_bytes(int64_t N, int64_t Fin);
int feature_count_run(hipStream_t stream, void* ws, size_t ws_bytes, const void* x, int64_t N, int64_t Fin, int flags, int64_t* nnz);
// arena bytes of the build, and the build; fills *desc on success; returns an RLAP_* status
size_t feature_build_bytes(int64_t N, int64_t Fin, int flags);
int feature_build_run(hipStream_t stream, void* ws, size_t ws_bytes, const FeatureBuildArgs& a, rlap_feature_desc* desc, FeatureReport* rep);
// arena bytes of a planned call, and the call (no host synchronisation)
size_t feature_apply_bytes(const rlap_feature_desc& d, int64_t K, int64_t Fout, int flags, int64_t part_limit);
int feature_apply_run(hipStream_t stream, void* ws, size_t ws_bytes, const FeatureApplyArgs& a);

}  // namespace rlap
