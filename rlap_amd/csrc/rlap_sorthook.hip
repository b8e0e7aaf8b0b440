// rlap_sorthook.hip -- the test hook of the sorts in rlap_wave_sort.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rlap_core.h"
#include "rlap_kernels.h"
#include "rlap_wave_sort.h"

namespace rlap {

struct RecKeyLessDbg { const SRec* r; __device__ bool operator()(uint16_t a, uint16_t b) const { return r[a].key < r[b].key; } };
struct RecKeyGreaterDbg { const SRec* r; __device__ bool operator()(uint16_t a, uint16_t b) const { return r[a].key > r[b].key; } };
// test hook: one wave sorts one array of doubles, returns the permutation (tests/test_gpu_parity.py).
// It has a translation unit of its own so that it can call any sort instantiation without touching the code of the kernels that use it.
__global__ __launch_bounds__(64) void k_debug_wave_sort(const double* __restrict__ keys, const int32_t* __restrict__ offs, int32_t narr,
                                                        int32_t desc, int32_t* __restrict__ perm_out) {
    __shared__ SRec rec[SCAP];
    __shared__ WaveSortScratch W;
    __shared__ int32_t tmp64[160];
    __shared__ uint32_t ltab[SCAP];
    __shared__ uint16_t ltab2[SCAP];
    const int lane = lane_id();
    for (int32_t arr = blockIdx.x; arr < narr; arr += gridDim.x) {
        const int32_t o = offs[arr], n = offs[arr + 1] - o;
        for (int q = lane; q < n; q += 64) { rec[q].key = keys[o + q]; rec[q].idx = q; rec[q].aux = 0; }
        __syncthreads();
        WaveSortPtrs WP = {W.ulist, W.dlist, W.segmark, W.stk};
        if (desc & 4) {   // half-wave variant: this block's wave sorts arrays 2*arr and 2*arr+1 side by side (those of <= 32 elements)
            const int32_t a2 = 2 * arr + (lane >> 5);
            const int gl = lane & 31;
            int32_t o2 = 0, n2 = 0;
            if (a2 < narr) { o2 = offs[a2]; n2 = offs[a2 + 1] - o2; }
            const bool want = a2 < narr && n2 <= 32 && n2 >= 1;
            double key = (want && gl < n2) ? keys[o2 + gl] : 0.0;
            int idx = gl, pos = gl;
            bool ok = (desc & 1) ? group_sort<true, 32>(key, idx, n2, want, lane, tmp64, &pos) : group_sort<false, 32>(key, idx, n2, want, lane, tmp64, &pos);
            if (want && gl < n2) perm_out[o2 + (ok ? pos : gl)] = ok ? idx : -1;
            __syncthreads();
            if (2 * arr + 2 >= narr) break;
            continue;
        }
        if ((desc & 2) && n <= 64) {   // register-resident variant (batch candidates of the 64-slot kernel)
            double key = lane < n ? rec[lane].key : 0.0;
            int idx = lane, pos = lane;
            bool ok = (desc & 1) ? wave_sort64<true>(key, idx, n, lane, tmp64, &pos) : wave_sort64<false>(key, idx, n, lane, tmp64, &pos);
            if (lane < n) perm_out[o + (ok ? pos : lane)] = ok ? idx : -1;
            __syncthreads();
            continue;
        }
        if ((desc & 16) && n <= 128) {   // level-synchronous variant over an INDEX array, keys looked up by the comparison (128-slot candidates)
            __shared__ uint16_t ord[128];
            for (int q = lane; q < n; q += 64) ord[q] = (uint16_t)q;
            __syncthreads();
            const bool ok = (desc & 1) ? wave_lvl_sort<uint16_t, RecKeyGreaterDbg, 2>(ord, n, RecKeyGreaterDbg{rec}, W.ulist, W.dlist, ltab, ltab2, lane)
                                       : wave_lvl_sort<uint16_t, RecKeyLessDbg, 2>(ord, n, RecKeyLessDbg{rec}, W.ulist, W.dlist, ltab, ltab2, lane);
            __syncthreads();
            for (int q = lane; q < n; q += 64) perm_out[o + q] = ok ? (int32_t)ord[q] : -1;
            __syncthreads();
            continue;
        }
        if (desc & 8) {   // level-synchronous variant (single-vertex path, long columns of the output pass)
            bool ok;
            if (n <= 128) ok = (desc & 1) ? wave_lvl_sort<SRec, SRecGreaterKey, 2>(rec, n, SRecGreaterKey(), W.ulist, W.dlist, ltab, ltab2, lane) : wave_lvl_sort<SRec, SRecLessKey, 2>(rec, n, SRecLessKey(), W.ulist, W.dlist, ltab, ltab2, lane);
            else if (n <= 256) ok = (desc & 1) ? wave_lvl_sort<SRec, SRecGreaterKey, 4>(rec, n, SRecGreaterKey(), W.ulist, W.dlist, ltab, ltab2, lane) : wave_lvl_sort<SRec, SRecLessKey, 4>(rec, n, SRecLessKey(), W.ulist, W.dlist, ltab, ltab2, lane);
            else ok = (desc & 1) ? wave_lvl_sort<SRec, SRecGreaterKey, 8>(rec, n, SRecGreaterKey(), W.ulist, W.dlist, ltab, ltab2, lane) : wave_lvl_sort<SRec, SRecLessKey, 8>(rec, n, SRecLessKey(), W.ulist, W.dlist, ltab, ltab2, lane);
            if (!ok) {   // depth limit: start over on the original order
                __syncthreads();
                for (int q = lane; q < n; q += 64) { rec[q].key = keys[o + q]; rec[q].idx = q; rec[q].aux = 0; }
                __syncthreads();
                if (desc & 1) wave_std_sort<SRec>(rec, n, SRecGreaterKey(), WP, lane); else wave_std_sort<SRec>(rec, n, SRecLessKey(), WP, lane);
            }
        } else if (desc & 1) wave_std_sort<SRec>(rec, n, SRecGreaterKey(), WP, lane); else wave_std_sort<SRec>(rec, n, SRecLessKey(), WP, lane);
        __syncthreads();
        for (int q = lane; q < n; q += 64) perm_out[o + q] = rec[q].idx;
        __syncthreads();
    }
}

}  // namespace rlap
