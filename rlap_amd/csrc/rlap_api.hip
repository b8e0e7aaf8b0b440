// rlap_api.hip -- C ABI (include/rlap_hip.h) and host orchestration of the kernels.
// Host code here only sizes buffers, launches kernels on the handle's stream and
// reads back a few scalars; all arithmetic of the path runs in rlap_kernels.hip.
// rocPRIM (AMD's native primitives, header-only) supplies the device radix sort
// and prefix sums used for plumbing (COO ordering, offsets).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_core.h"
#include "rlap_kernels.h"
#include "rlap_cheb.h"
#include "rlap_snapshot.h"
#include "rlap_ppr.h"
#include "rlap_markov_api.h"
#include "rlap_stats.h"
#include "rlap_subgraph.h"
#include "rlap_gcn.h"
#include "rlap_plan.h"
#include "rlap_edgeplan.h"
#include "rlap_featlin_api.h"
#include "rlap_edgedrop.h"
#include "rlap_nodesample.h"
#include "rlap_edgeadd.h"
#include "rlap_spmm_api.h"
#include "rlap_spmm.h"
#include "rlap_readout.h"
#include "rlap_readout_api.h"
#include "rlap_infonce.h"
#include "rlap_infonce_api.h"
#include "rlap_g2l.h"
#include "rlap_g2l_api.h"
#include "rlap_cca.h"
#include "rlap_cca_api.h"
#include "rlap_bt.h"
#include "rlap_bt_api.h"
#include "rlap_linear.h"
#include "rlap_linear_api.h"
#include "rlap_norm.h"
#include "rlap_norm_api.h"
#include "rlap_rowops.h"
#include "rlap_rowops_api.h"
#include "rlap_probe.h"
#include "rlap_probe_api.h"

using namespace rlap;

namespace {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

#define ENSURE(buf, bytes) RLAP_HIPCHK((buf).ensure((size_t)(bytes)))

inline unsigned nblk(int64_t n, int bs) { return (unsigned)std::max<int64_t>(1, (n + bs - 1) / bs); }

}  // namespace

// Every per-call buffer is carved out of ONE arena (256-byte aligned pieces, the layout is a function of the host-known sizes E, n, G
// and the handle's growth factors).  The arena is either the caller's (rlap_set_workspace: torch's allocator in rlap_amd/ops.py -- the
// reference lets torch allocate what the op needs, py_api_binder.cc:42) or the handle's own (one hipMalloc, grown only when a call needs
// a larger size class than any before it).  The cached uniform table is a second, persistent buffer under the same rule.
struct rlap_handle_s {
    int device = 0;
    int n_cu = 0;                 // compute units of `device`
    bool big_attr_set = false;    // k_sc_merge_big's 128 KB dynamic-LDS opt-in (a per-device function attribute)
    std::mutex mu;                // one call at a time per handle (the workspace is the handle's); use one handle per host thread for concurrency
    hipStream_t stream = nullptr;
    bool timing = false;
    hipEvent_t ev[8];
    hipStream_t side[2] = {nullptr, nullptr};   // the output pass's independent tiers run side by side
    hipEvent_t fork_ev[3];
    // the arena: caller-provided (ext_ws) or owned
    void* ext_ws = nullptr; size_t ext_ws_bytes = 0;
    DevBuf own_ws;
    size_t ws_needed = 0;         // bytes the last call wanted (reported with RLAP_E_WORKSPACE)
    // the uniform table: caller-provided or owned; rng_len = entries generated so far in the current buffer
    double* ext_rng = nullptr; int64_t ext_rng_cap = 0;
    DevBuf own_rng;
    double* rng_ptr = nullptr;
    int64_t rng_len = 0;
    int64_t rng_needed = 0;       // entries the last call wanted
    DevBuf eqtab;   // k_eq_tables, allocated and built at rlap_create
    DevBuf small;   // two 64-bit words for rlap_approx_chol_from_edges' num_nodes reduction (max id + 1, negative-id flag)
    DevBuf prof;    // diagnostic phase profile (RLAP_PHASE_PROFILE=1), allocated at rlap_create
    DevBuf trace;   // diagnostic per-position time stamps of the dataflow kernel (RLAP_FLOW_TRACE=<file>)
    // pinned host mirror of what a call reads back
    void* h_results = nullptr; size_t h_results_cap = 0;
    // growth factors kept across calls
    double pool_factor = 1.0;
    double log_factor = 2.0;
    int64_t rng_min = 0;          // lower bound of the uniform table (grown after an overflow)
    int64_t scr_budget = 1 << 18; // output pass: entries of global scratch for columns beyond 8192 slots
    double flow_scr_factor = 1.0; // dataflow elimination: working storage of the long columns (grown after ST_FLOW_SCRATCH)
    bool flow_off_once = false;   // the next attempt uses the round kernel (set after ST_FLOW_REORDER, or after the dataflow kernel gave up)
    int rng_mode = 0;             // 0 the reference's one stream (mode "exact"), 1 counter-based uniforms (mode "frontier", rlap_set_rng_mode)
    // test hooks (rlap_debug_set_limits): tiny first sizes so that the retry path runs
    double dbg_pool = -1.0, dbg_log = -1.0; int64_t dbg_rng = -1, dbg_scr = -1;
    int64_t dbg_ro_cap = -1;      // (rlap_debug_set_flow_limits) entries of the dataflow reorder buffer, first attempt of the next call only
    int64_t total_retries = 0;
    bool force_sort = false;      // the next attempt sorts the COO whatever order it is in (set when a skipped sort cannot be trusted)
    int jitter = 0;               // RLAP_DEBUG_JITTER=<n>: waves of the elimination kernel sleep n x 0.25 us behind its barriers (a different set each time)
    int poison = -1;              // RLAP_DEBUG_POISON=<byte>: the arena, the output buffer and the elimination kernel's LDS are filled with it before every attempt
};

namespace {

// The arena of a call that wants `need` bytes: the caller's (rlap_set_workspace) or the handle's own, grown when it is too small.
// ws_needed is set first: RLAP_E_WORKSPACE is answered by rlap_workspace_needed().
int arena(rlap_handle h, size_t need, void** base, size_t* have) {
    h->ws_needed = need;
    if (h->ext_ws) {
        if (need > h->ext_ws_bytes) return RLAP_E_WORKSPACE;   // the caller allocates rlap_workspace_needed() bytes and calls again
        *base = h->ext_ws; *have = h->ext_ws_bytes;
    } else {
        ENSURE(h->own_ws, need);
        *base = h->own_ws.p; *have = h->own_ws.cap;
    }
    return RLAP_OK;
}

// device-side scalars of a call, zeroed by one memset
struct Scalars {
    int32_t flags[FLAG_COUNT];
    int32_t nnz; int32_t pad;
    double acc[4];
    unsigned long long counters[8];   // [0] sc scratch top, [4..6] tier counts (6 ints)
    unsigned long long maxid;
    unsigned long long live[LIVE_SLOTS * LIVE_STRIDE];   // live entries read by the output pass, partial sums
};

// The first `count` uniforms of the sampling stream (K10) in the handle's table.  The table lives in the caller's buffer
// (rlap_set_rng_table) or in the handle's own; it is generated from the start whenever the buffer changes or must grow.
int ensure_rng(rlap_handle h, int64_t count) {
    h->rng_needed = std::max<int64_t>(count, 1 << 16);
    if (h->rng_ptr && count <= h->rng_len) return RLAP_OK;
    int64_t want = h->rng_needed;
    double* buf = nullptr;
    if (h->ext_rng) {
        if (want > h->ext_rng_cap) return RLAP_E_WORKSPACE;
        buf = h->ext_rng; want = h->ext_rng_cap;
    } else {
        ENSURE(h->own_rng, sizeof(double) * (size_t)want);
        buf = h->own_rng.as<double>(); want = (int64_t)(h->own_rng.cap / sizeof(double));
    }
    hipLaunchKernelGGL(k_mt19937_64_table, dim3(1), dim3(320), 0, h->stream, buf, want);
    RLAP_HIPCHK(hipGetLastError());
    h->rng_ptr = buf; h->rng_len = want;
    return RLAP_OK;
}

// temporary storage of the rocPRIM calls: sized up front (queries with a null pointer touch nothing) and carved from the arena
struct SortTmp { void* p; size_t bytes; };

template <class K, class V>
int sort_pairs(rlap_handle h, const SortTmp& T, K* k_in, K* k_out, V* v_in, V* v_out, int64_t n, unsigned begin_bit, unsigned end_bit) {
    size_t bytes = 0;
    RLAP_HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, k_in, k_out, v_in, v_out, (size_t)n, begin_bit, end_bit, h->stream));
    if (bytes > T.bytes) return RLAP_E_INTERNAL;   // (sort_tmp_bytes asks the same questions up front)
    bytes = T.bytes;
    RLAP_HIPCHK(rocprim::radix_sort_pairs(T.p, bytes, k_in, k_out, v_in, v_out, (size_t)n, begin_bit, end_bit, h->stream));
    return RLAP_OK;
}

template <class In, class Out>
int excl_scan(rlap_handle h, const SortTmp& T, In* in, Out* out, int64_t n) {
    size_t bytes = 0;
    RLAP_HIPCHK(rocprim::exclusive_scan(nullptr, bytes, in, out, (Out)0, (size_t)n, rocprim::plus<Out>(), h->stream));
    if (bytes > T.bytes) return RLAP_E_INTERNAL;
    bytes = T.bytes;
    RLAP_HIPCHK(rocprim::exclusive_scan(T.p, bytes, in, out, (Out)0, (size_t)n, rocprim::plus<Out>(), h->stream));
    return RLAP_OK;
}

inline unsigned bits_for(uint64_t maxval) { unsigned b = 1; while (b < 64 && (maxval >> b) != 0) ++b; return b; }

// largest temporary any rocPRIM call of a call with these sizes asks for (the very calls run_once makes, asked with null storage)
int sort_tmp_bytes(int64_t Eeff, int64_t N, int64_t G, int64_t S, bool flow, size_t* out) {
    size_t mx = 256, b = 0;
    hipStream_t s0 = nullptr;
    const unsigned kbits = bits_for((uint64_t)(N > 1 ? N - 1 : 1)), gbits = bits_for((uint64_t)(G > 0 ? G - 1 : 0));
    if (Eeff > 0) {
        b = 0; RLAP_HIPCHK(rocprim::radix_sort_pairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)Eeff, 0u, std::min(64u, 2 * kbits + 1), s0)); mx = std::max(mx, b);
        rocprim::counting_iterator<uint32_t> iota(0u);
        b = 0; RLAP_HIPCHK(rocprim::radix_sort_pairs(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, iota, (uint32_t*)nullptr, (size_t)Eeff, 0u, std::min(32u, kbits + 1), s0)); mx = std::max(mx, b);
        b = 0; RLAP_HIPCHK(rocprim::exclusive_scan(nullptr, b, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)(Eeff + 1), rocprim::plus<int32_t>(), s0)); mx = std::max(mx, b);
    }
    const size_t Nn = (size_t)std::max<int64_t>(N, 1);
    b = 0; RLAP_HIPCHK(rocprim::radix_sort_pairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, Nn, 0u, 32u + gbits, s0)); mx = std::max(mx, b);
    b = 0; RLAP_HIPCHK(rocprim::radix_sort_pairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, Nn, 0u, 64u, s0)); mx = std::max(mx, b);
    b = 0; RLAP_HIPCHK(rocprim::exclusive_scan(nullptr, b, (int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(S + 1), rocprim::plus<int64_t>(), s0)); mx = std::max(mx, b);
    if (flow && Eeff > 0) {   // tag order of the surviving columns (rlap_flow.hip): one (column, tag) sort over at most Eeff appended entries
        b = 0; RLAP_HIPCHK(rocprim::radix_sort_pairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)Eeff, 0u, 64u, s0)); mx = std::max(mx, b);
        b = 0; RLAP_HIPCHK(rocprim::exclusive_scan(nullptr, b, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t)0, (size_t)(S + 1), rocprim::plus<int32_t>(), s0)); mx = std::max(mx, b);
    }
    *out = mx;
    return RLAP_OK;
}

// o_v = random runs the dataflow kernel (rlap_flow.hip) unless RLAP_FLOW=0 asks for the round kernel.  Default: single graphs and
// pairs, and batches of up to 64 graphs of 1024 vertices or more on average -- there the waves of the whole device work on few graphs
// (BA(4096,8), ms per call, round kernel / dataflow: 4 graphs 9.5 / 4.6, 16: 10.1 / 6.0, 32: 10.6 / 7.4, 64: 9.7-15.8 / 9.2, 96: 11.4 /
// 11.1, 128: 11.7 / 12.4, 1024: 30 / 59).  A batch of many graphs is bound by the positions in flight, where one workgroup per graph
// with a round's loads all in flight together does better.  RLAP_FLOW=1 forces the dataflow kernel for any batch.
inline bool flow_wanted(const rlap_handle h, int o_v, int64_t G, int64_t n_total) {
    if (o_v != OV_RANDOM || h->flow_off_once) return false;
    const char* e = std::getenv("RLAP_FLOW");
    if (e && e[0] == '0') return false;
    if (e && e[0] == '1') return true;
    return G <= 2 || (G <= 64 && n_total >= 1024 * G);
}

constexpr int64_t SORT_SKIP_MIN = 1 << 21;   // directed entries from which the order of the input is looked at before sorting it

struct Fills {
    FillJobs J; int64_t maxcount = 0;
    Fills() { J.n = 0; }
    void add(void* p, int64_t count_i32, int32_t v) { if (count_i32 <= 0) return; J.ptr[J.n] = (int32_t*)p; J.count[J.n] = count_i32; J.value[J.n] = v; ++J.n; maxcount = std::max(maxcount, count_i32); }
    void launch(hipStream_t s) {
        if (J.n == 0) return;
        unsigned gx = (unsigned)std::min<int64_t>((maxcount + 255) / 256, 2048);
        hipLaunchKernelGGL(k_fill_multi, dim3(gx, (unsigned)J.n), dim3(256), 0, s, J);
        J.n = 0; maxcount = 0;
    }
};

// keyed random permutation of each graph's local ids, drawn on the device (stands in for the
// std::shuffle(random_device) of preconditioner.cc:594-596 when the caller injects no node_id vector).
// Graph g of a batch is keyed by seed + g like the neighbour order (rlap_core.h): a batched or sharded call draws what
// single-graph calls with seed + g draw, whatever the sharding.  64 hash bits: no ties to break at any graph size.
__global__ void k_perm_keys(const int32_t* __restrict__ vgraph, const GraphDesc* __restrict__ gd, int32_t N, uint64_t seed, int gbits,
                            uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int32_t g = vgraph[i];
    const uint32_t local = (uint32_t)(i - gd[g].vbase);
    const uint64_t hk = mix64(mix64((seed + (uint64_t)g) ^ 0x7065726D5F6B6579ull) ^ mix64(local));
    // one graph: the whole hash; a batch: the graph number on top of 64 - gbits hash bits (one 64-bit sort either way)
    keys[i] = gbits == 0 ? hk : (((uint64_t)(uint32_t)g << (64 - gbits)) | (hk >> gbits));
    vals[i] = local;
}
__global__ void k_widen_u32(const uint32_t* __restrict__ in, int32_t N, int64_t* __restrict__ out) {
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N) out[i] = (int64_t)in[i];
}

// Depths call (rlap_approx_chol_depths, rlap_approx_chol_views_depths): before segment k, graph j's num_remove becomes t_k[j] (row k
// of the depth table, [D][G]; the round kernel runs to it) and, for the dataflow kernel, whose positions were all queued up front,
// n_elim becomes the snapshot's, min(t_k[j], n_j - 1) (k_sc_perm_order reads it).  `resume` (round kernel): 0 for the first segment,
// 1 for the later ones, which continue from the n_elim the previous one left.  One thread per graph.
__global__ void k_depth_set(GraphDesc* __restrict__ gd, const int64_t* __restrict__ t_row, int32_t G, int32_t set_n_elim, int32_t resume) {
    const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= G) return;
    const int64_t t = t_row[j];
    gd[j].t = t;
    if (set_n_elim) { const int64_t n = gd[j].n; gd[j].n_elim = (int32_t)(t < 0 ? 0 : (t < n - 1 ? t : (n > 0 ? n - 1 : 0))); }
    gd[j].resume = resume;
}
// After a segment's elimination: any graph's failure stops the call's later work (sticky; k_sc_ext stages nothing, k_flow_segment
// starts no claim).  A graph that failed keeps the n_elim of the segment it failed in, so the host's survivor bases of later
// snapshots no longer describe it.
__global__ void k_depth_stop(const GraphDesc* __restrict__ gd, int32_t G, int32_t* __restrict__ stop) {
    int32_t st = 0;
    for (int32_t j = threadIdx.x; j < G; j += blockDim.x) st |= gd[j].status;
    if (st) atomicOr(stop, 1);
}
// Dataflow kernel, batches: the claim order sorted by (position, graph) is regrouped by segment, so that segment k is the contiguous
// claim range [Q_{k-1}, Q_k).  Key of a claim = the segment its position falls in (first k with p < n_elim of depth k); the radix
// sort over it is stable, so each segment keeps the interleaved (position, graph) order, and with it each graph's own order.
__global__ void k_flow_seg_keys(const uint32_t* __restrict__ qorder, int32_t Q, const int32_t* __restrict__ qg, const GraphDesc* __restrict__ gd,
                                const int64_t* __restrict__ t_tab, int32_t D, int32_t G, uint64_t* __restrict__ keys) {
    const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q) return;
    const int32_t li = (int32_t)qorder[i];
    const int32_t g = qg[li];
    const int64_t p = (int64_t)(li - gd[g].flow_base - 1);
    const int64_t n = gd[g].n;
    int32_t lo = 0, hi = D - 1;   // the deepest depth queued every position: the answer is in [0, D-1]
    while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        const int64_t t = t_tab[(int64_t)mid * G + g];
        const int64_t ne = t < 0 ? 0 : (t < n - 1 ? t : n - 1);
        if (p < ne) hi = mid; else lo = mid + 1;
    }
    keys[i] = (uint64_t)lo;
}
// After snapshot k's output pass: graph j's rows end at ptr[kG + j + 1] = ptr[kG] + row_off[sb[j + 1]] (sb: the snapshot's survivor
// bases, ptr[kG] filed by the previous snapshot); the output pass's counters (scratch top, tier counts, live entries) start from 0
// for the next snapshot, whose ext / cnt sentinels (index S_next) are zeroed.  The largest scratch top any snapshot asked for is kept
// and handed to k_collect by the last one (S_next < 0), so that a scratch retry grows enough.
__global__ void k_depth_close(const int64_t* __restrict__ row_off, const int64_t* __restrict__ sb, int32_t G, int64_t* __restrict__ out_ptr,
                              unsigned long long* __restrict__ counters, unsigned long long* __restrict__ live, unsigned long long* __restrict__ scr_max,
                              int32_t S_next, int32_t* __restrict__ ext, int32_t* __restrict__ cnt) {
    const int tid = threadIdx.x;
    const int64_t base = out_ptr[0];
    for (int32_t j = tid; j < G; j += blockDim.x) out_ptr[j + 1] = base + row_off[sb[j + 1]];
    if (tid == 0) {
        const unsigned long long m = counters[0] > *scr_max ? counters[0] : *scr_max;
        if (S_next >= 0) {
            *scr_max = m;
            for (int q = 0; q < 8; ++q) counters[q] = 0ull;
            ext[S_next] = 0; cnt[S_next] = 0;
        } else counters[0] = m;
    }
    if (S_next >= 0) for (int q = tid; q < LIVE_SLOTS * LIVE_STRIDE; q += blockDim.x) live[q] = 0ull;
}

// Host-known sizes of one call (upper bounds; what only the device knows -- nnz, row counts -- never sizes a buffer).
struct Sizes {
    int64_t G, N, Eeff, slot_cap, bucket_total, log_total, scr_total, S, scr_budget;
    size_t sort_tmp, res_bytes;
    bool want_genperm;
    bool flow;                    // dataflow elimination (o_v = random): its arrays are part of the arena
    int64_t flow_Q, flow_scr;     // look-back words (positions + one sentinel per graph); entries of long-column working storage
    int64_t D;                    // depths call: snapshots (0 otherwise)
    int squeeze;                  // squeeze passes of the degree order (0: none): a second entry arena and the pass's arrays are part of the arena
};
struct WBuf { void* p = nullptr; template <class T> T* as() const { return reinterpret_cast<T*>(p); } };
struct WS {
    WBuf node_ptr_d, depth_t, depth_sb, vgraph, scal, keys0, keys1, idx0, idx1, head, pos, sorttmp, colptr, slot_col, permchk, genperm, ent, vrec, ocur, oend, origpos, orig_order, gd_d, pool_top, bs_cnt, bs_alloc, bs_dir, bs_v, bs_id, bs_pool_top, batch_pos, skey0, skey1, sval0, sval1, scr_rec, scr_i32, scr_f64, surv_base_d, ext, tmp_off, tmp_nbr, tmp_val, cnt, row_off, sc_rec, sc_i32, sc_f64, biglist, hugelists, results,
         f_cdir, f_atag, f_lb, f_qv, f_qg, f_ctrl, f_scr, f_rocnt, f_rooff,
         sq_ent, sq_colptr, sq_rank, sq_cnt, sq_list, sq_nlong, sq_marks;
};
// depths call (D > 0): the depth table t[D][G] and every snapshot's survivor bases sb[D][G + 1] follow
inline size_t host_block_bytes(int64_t G, int64_t D) {
    return 16 * (size_t)(G + 1) + sizeof(GraphDesc) * (size_t)G + (D > 0 ? 8 * (size_t)D * (size_t)(2 * G + 1) : 0);
}
// the arena's layout: run once with a null base to learn the size, once more to place the buffers
size_t carve(Carve& C, const Sizes& z, WS& W) {
    const int64_t G = z.G, N = z.N, S = z.S, Ealloc = std::max<int64_t>(z.Eeff, 1), BT = z.bucket_total;
    W.scal.p = C.take<Scalars>(1);
    W.results.p = C.take<char>((int64_t)z.res_bytes);
    {   // what the host hands over per call, one block (one H2D copy from the pinned staging buffer): node_ptr | surv_base | gd
        // (| depth table | snapshot survivor bases)
        char* hp = C.take<char>((int64_t)host_block_bytes(G, z.D));
        W.node_ptr_d.p = hp;
        W.surv_base_d.p = hp ? hp + 8 * (G + 1) : nullptr;
        W.gd_d.p = hp ? hp + 16 * (G + 1) : nullptr;
        char* dp = hp ? hp + 16 * (G + 1) + sizeof(GraphDesc) * G : nullptr;
        W.depth_t.p = z.D > 0 ? dp : nullptr;
        W.depth_sb.p = z.D > 0 && dp ? dp + 8 * z.D * G : nullptr;
    }
    W.pool_top.p = C.take<int32_t>(1);
    W.bs_pool_top.p = C.take<int32_t>(1);
    W.vgraph.p = C.take<int32_t>(N);
    W.keys0.p = C.take<uint64_t>(Ealloc); W.keys1.p = C.take<uint64_t>(Ealloc);
    W.idx0.p = C.take<uint32_t>(Ealloc); W.idx1.p = C.take<uint32_t>(Ealloc);
    W.head.p = C.take<int32_t>(Ealloc + 1); W.pos.p = C.take<int32_t>(Ealloc + 1);
    W.sorttmp.p = C.take<char>((int64_t)z.sort_tmp);
    W.ent.p = C.take<Slot>(z.slot_cap);
    W.slot_col.p = C.take<int32_t>(Ealloc);
    W.colptr.p = C.take<int32_t>(N + 1);
    W.vrec.p = C.take<VRec>(N);
    W.origpos.p = C.take<int32_t>(N);
    W.ocur.p = C.take<int32_t>(BT); W.oend.p = C.take<int32_t>(BT);
    W.bs_cnt.p = C.take<int32_t>(BT); W.bs_alloc.p = C.take<int32_t>(BT); W.bs_dir.p = C.take<int32_t>(BT * BDIR);
    W.bs_v.p = C.take<int32_t>(z.log_total); W.bs_id.p = C.take<int32_t>(z.log_total);
    W.batch_pos.p = C.take<int32_t>(N);
    W.skey0.p = C.take<uint64_t>(N); W.skey1.p = C.take<uint64_t>(N); W.sval0.p = C.take<uint32_t>(N); W.sval1.p = C.take<uint32_t>(N);
    W.orig_order.p = C.take<int32_t>(N);
    W.permchk.p = C.take<int32_t>(N);
    W.genperm.p = C.take<int64_t>(z.want_genperm ? N : 0);
    W.scr_rec.p = C.take<SRec>(z.scr_total); W.scr_i32.p = C.take<int32_t>(10 * z.scr_total); W.scr_f64.p = C.take<double>(4 * z.scr_total);
    W.ext.p = C.take<int32_t>(S + 1); W.cnt.p = C.take<int32_t>(S + 1); W.tmp_off.p = C.take<int64_t>(S + 1); W.row_off.p = C.take<int64_t>(S + 1);
    W.tmp_nbr.p = C.take<int32_t>(z.slot_cap); W.tmp_val.p = C.take<double>(z.slot_cap);   // staged rows: at most one per slot in use
    W.sc_rec.p = C.take<SRec>(z.scr_budget); W.sc_i32.p = C.take<int32_t>(7 * z.scr_budget); W.sc_f64.p = C.take<double>(2 * z.scr_budget);
    W.biglist.p = C.take<int32_t>(8 * (S + 1));
    W.hugelists.p = C.take<uint16_t>((int64_t)NHUGE * 2 * (HUGECAP + 2));
    if (z.flow) {
        W.f_ctrl.p = C.take<int32_t>(FC_WORDS);
        W.f_cdir.p = C.take<int32_t>(N * FDIR);
        W.f_atag.p = C.take<int32_t>(z.slot_cap);
        W.f_lb.p = C.take<unsigned long long>(z.flow_Q); W.f_qv.p = C.take<int32_t>(z.flow_Q); W.f_qg.p = C.take<int32_t>(z.flow_Q);
        W.f_scr.p = C.take<char>(z.flow_scr * FLOW_SCR_BYTES);
        W.f_rocnt.p = C.take<int32_t>(S + 1); W.f_rooff.p = C.take<int32_t>(S + 1);
    }
    if (z.squeeze > 0) {   // 20 bytes per slot and 12 per vertex on top (rlap_squeeze.h)
        W.sq_ent.p = C.take<Slot>(z.slot_cap);
        W.sq_rank.p = C.take<int32_t>(z.slot_cap);
        W.sq_colptr.p = C.take<int32_t>(N + 1); W.sq_cnt.p = C.take<int32_t>(N + 1); W.sq_list.p = C.take<int32_t>(N);
        W.sq_nlong.p = C.take<int32_t>(1);
        W.sq_marks.p = C.take<int32_t>((int64_t)z.squeeze * G);
    }
    return (C.off + 255) & ~(size_t)255;
}

// sizes of a call on (E directed input entries, N vertices, G graphs, S surviving vertices) under the handle's growth factors
// `segs` > 0 (depths call, that many segments): the round kernel reserves a fresh block of pool slots per graph in every segment, the
// host block carries the depth table and the snapshots' survivor bases, and the read-back block holds segs * G + 1 row pointers, the
// scratch maximum and the stop word
int call_sizes(const rlap_handle h, int64_t Eeff, int64_t N, int64_t G, int64_t bucket_total, int64_t S, bool want_genperm, bool flow, int64_t nelim_total, Sizes* z,
               int64_t segs = 0, int squeeze = 0) {
    const double pool_factor = h->dbg_pool >= 0 ? h->dbg_pool : h->pool_factor;
    const double log_factor = h->dbg_log >= 0 ? h->dbg_log : h->log_factor;
    const int64_t nnz_ub = Eeff;
    const int64_t pool = (int64_t)(pool_factor * nnz_ub) + (h->dbg_pool >= 0 ? 0 : 16 * N + 1024) + G * std::max<int64_t>(segs, 1) * (G <= 512 ? (int64_t)POOL_GRAB_BIG : (int64_t)POOL_GRAB_SMALL);
    z->G = G; z->N = N; z->Eeff = Eeff; z->S = S; z->bucket_total = bucket_total;
    z->slot_cap = nnz_ub + pool;
    if (z->slot_cap >= ((int64_t)1 << 31) - 64) return RLAP_E_TOO_LARGE;
    z->log_total = (int64_t)(log_factor * nnz_ub) + (h->dbg_log >= 0 ? 64 : (int64_t)BCH0 * bucket_total + 64 * G);
    z->scr_total = nnz_ub / 2 + 8 * G + 8;
    if (bucket_total * BDIR >= ((int64_t)1 << 40) || bucket_total >= ((int64_t)1 << 31) || z->log_total >= ((int64_t)1 << 31)) return RLAP_E_TOO_LARGE;
    z->scr_budget = h->dbg_scr >= 0 ? h->dbg_scr : h->scr_budget;
    z->res_bytes = sizeof(CallResults) + 8 * (size_t)(G + 1) + (segs > 0 ? 8 * (size_t)(segs * G + 3) : 0);
    z->D = segs;
    z->want_genperm = want_genperm;
    z->flow = flow;
    z->squeeze = squeeze;
    z->flow_Q = nelim_total + G;
    z->flow_scr = flow ? (int64_t)(h->flow_scr_factor * (double)std::max<int64_t>(Eeff / 16, 1 << 17)) : 0;
    if (flow && h->dbg_scr >= 0) z->flow_scr = std::max<int64_t>(h->dbg_scr, 16);   // (test hook: a tiny first size, so that the retry runs)
    if (z->flow_scr >= ((int64_t)1 << 31) - 64) z->flow_scr = ((int64_t)1 << 31) - 64;
    { int rc = sort_tmp_bytes(Eeff, N, G, S, flow, &z->sort_tmp); if (rc) return rc; }
    if (squeeze > 0) {   // the pass's prefix sum over the N + 1 live counts shares the temporary storage
        size_t b = 0;
        RLAP_HIPCHK((hipError_t)squeeze_scan_tmp_bytes(N, &b));
        z->sort_tmp = std::max(z->sort_tmp, b);
    }
    return RLAP_OK;
}

// uniforms a call may draw: a graph rarely draws more than its own directed entry count; an overflow doubles the table
int64_t rng_guess(const rlap_handle h, int64_t Eeff, int64_t G) {
    int64_t guess = (G == 1) ? Eeff + 1024 : std::min<int64_t>(Eeff + 1024, 4 * (Eeff / G) + 65536);
    return std::max<int64_t>(std::max(guess, h->rng_min), 1 << 16);
}

struct Call {
    const int64_t* d_row; const int64_t* d_col; const double* d_w; int64_t E;
    int64_t G; const int64_t* h_node_ptr; const int64_t* h_t;
    int o_v, o_n; const int64_t* d_perm; uint64_t seed;
    double* d_out; int64_t out_cap; int64_t* h_out_row_ptr; rlap_stats* st;
    int symmetrize;
    int64_t K = 1;   // views (rlap_approx_chol_views): h_node_ptr / h_t describe the K-fold union, the device input is ONE copy of it
    // depths (rlap_approx_chol_depths / _views_depths): h_depths[D][G], each column non-decreasing, h_t = its last row
    const int64_t* h_depths = nullptr; int64_t D = 0;
};

// One attempt.  No host synchronisation until the single read-back at the end: every size is an upper bound
// known on the host (E, N, G); what only the device knows (nnz, row counts, overflows, input checks) is read
// by the kernels from device memory and reported once.
int run_once(rlap_handle h, const Call& c, int* retry_kind, int64_t* retry_need, int32_t* flow_abort) {
    *retry_kind = 0; *retry_need = 0; *flow_abort = 0;
    hipStream_t s = h->stream;
    const int64_t G = c.G, E = c.E;
    const int64_t N = c.h_node_ptr[G];
    // A views call is the batch of K copies of the input (G1 graphs, N1 vertices, E1eff entries): the COO -> CSR setup runs on the
    // one copy the caller gave, k_views_replicate then writes the union's CSR; everything after it sees the K * G1-graph batch.
    const int64_t K = c.K, G1 = G / K, N1 = N / K;
    const int64_t E1eff = c.symmetrize ? 2 * E : E;
    const int64_t Eeff = K * E1eff;
    if (N >= (int64_t)1 << 30 || Eeff >= (int64_t)1 << 31 || G >= (int64_t)1 << 30) return RLAP_E_TOO_LARGE;
    if (h->timing) RLAP_HIPCHK(hipEventRecord(h->ev[0], s));

    rlap_stats st;
    std::memset(&st, 0, sizeof(st));

    if (N == 0) {
        const int64_t nptr = c.D > 0 ? c.D * G : G;
        for (int64_t g = 0; g <= nptr; ++g) c.h_out_row_ptr[g] = 0;
        if (c.st) *c.st = st;
        return RLAP_OK;
    }

    // ---------------- sizes (host-known upper bounds) ----------------
    const int64_t nnz_ub = Eeff;
    std::vector<GraphDesc> gd((size_t)G);
    int64_t bucket_total = 0, nelim_total = 0;
    std::vector<int64_t> surv_base((size_t)G + 1, 0);
    for (int64_t g = 0; g < G; ++g) {
        GraphDesc& D = gd[g];
        std::memset(&D, 0, sizeof(D));
        int64_t n = c.h_node_ptr[g + 1] - c.h_node_ptr[g];
        D.vbase = (int32_t)c.h_node_ptr[g]; D.n = (int32_t)n; D.t = c.h_t[g];
        D.bucket_base = (int32_t)bucket_total; bucket_total += 2 * n + 1;
        int64_t ne = std::max<int64_t>(0, std::min<int64_t>(c.h_t[g], n - 1));
        D.n_elim = (int32_t)ne;
        D.flow_base = (int32_t)(nelim_total + g);
        nelim_total += ne;
        surv_base[g + 1] = surv_base[g] + (n - ne);
    }
    const int64_t S = surv_base[G];
    // depths call: segment k eliminates positions [ne[k-1][j], ne[k][j]) of every graph j; snapshot k has the survivor bases
    // sb[k][j] (sb[k][G] = S_k = N - Q_k, Q_k = the positions of depth k over all graphs; the first snapshot is the largest)
    const bool depths = c.D > 0;
    const int64_t nseg = depths ? c.D : 1;
    std::vector<int64_t> seg_Q((size_t)nseg, nelim_total), seg_sb;
    if (depths) {
        seg_sb.assign((size_t)(nseg * (G + 1)), 0);
        for (int64_t k = 0; k < nseg; ++k) {
            int64_t q = 0;
            int64_t* sb = seg_sb.data() + k * (G + 1);
            for (int64_t g = 0; g < G; ++g) {
                const int64_t n = c.h_node_ptr[g + 1] - c.h_node_ptr[g];
                const int64_t ne = std::max<int64_t>(0, std::min<int64_t>(c.h_depths[k * G + g], n - 1));
                q += ne;
                sb[g + 1] = sb[g] + (n - ne);
            }
            seg_Q[(size_t)k] = q;
        }
    }
    const int64_t S0 = depths ? N - seg_Q[0] : S;
    st.n_eliminated = nelim_total;
    Sizes z;
    const bool flow = flow_wanted(h, c.o_v, G, N);
    st.elim_kernel = nelim_total > 0 ? (flow ? 2 : 1) : 0;
    // degree order on a large graph: squeeze passes between launches of the 16-slot kernel (rlap_squeeze.h; 0: none)
    const int squeeze = flow ? 0 : squeeze_passes(c.o_v, (unsigned)G, h->n_cu, depths, c.K > 1, Eeff);
    { int rc = call_sizes(h, Eeff, N, G, bucket_total, S0, c.o_v == OV_RANDOM && !c.d_perm, flow, nelim_total, &z, depths ? nseg : 0, squeeze); if (rc) return rc; }
    const int64_t slot_cap = z.slot_cap, log_total = z.log_total, scr_total = z.scr_total, scr_budget = z.scr_budget;
    const size_t res_bytes = z.res_bytes;

    // ---------------- workspace: one arena, no allocation unless this call is of a larger size class than any before ----------------
    WS W;
    {
        Carve dry{nullptr, 0};
        const size_t need = carve(dry, z, W);
        void* base = nullptr;
        size_t have = 0;
        { int rc = arena(h, need, &base, &have); if (rc) return rc; }
        Carve real{static_cast<char*>(base), 0};
        carve(real, z, W);
        if (h->poison >= 0) {   // debug: whatever a kernel reads without having been given it is this byte, not the previous call's data
            RLAP_HIPCHK(hipMemsetAsync(base, h->poison, need, s));
            if (c.d_out && c.out_cap > 0) RLAP_HIPCHK(hipMemsetAsync(c.d_out, h->poison, sizeof(double) * 3 * (size_t)c.out_cap, s));
        }
    }
    {
        const size_t pinned_need = ((res_bytes + 255) & ~(size_t)255) + host_block_bytes(G, z.D);   // read-back block + staging of the host parameters
        if (pinned_need > h->h_results_cap) {
            if (h->h_results) (void)hipHostFree(h->h_results);
            h->h_results = nullptr; h->h_results_cap = 0;
            RLAP_HIPCHK(hipHostMalloc(&h->h_results, pinned_need + 65536, hipHostMallocDefault));
            h->h_results_cap = pinned_need + 65536;
        }
    }
    { int rc = ensure_rng(h, rng_guess(h, Eeff, G)); if (rc) return rc; }
    const SortTmp ST{W.sorttmp.p, z.sort_tmp};
    // (test hook: the kernels are told the table is shorter than it is)
    const int64_t rng_len_eff = h->dbg_rng >= 0 ? std::min<int64_t>(h->rng_len, h->dbg_rng) : h->rng_len;

    Scalars* SC = W.scal.as<Scalars>();
    int32_t* flags = SC->flags;
    double* acc = SC->acc;
    unsigned long long* counters = SC->counters;   // [0] sc scratch top
    unsigned long long* live = SC->live;
    int32_t* nnz_p = &SC->nnz;

    // ---------------- setup: COO -> CSR ----------------
    {
        // node_ptr | surv_base | gd: staged in pinned host memory (behind the read-back block), ONE asynchronous copy -- three copies
        // from pageable memory were three blocking staging copies inside the runtime
        char* stage = static_cast<char*>(h->h_results) + ((res_bytes + 255) & ~(size_t)255);
        std::memcpy(stage, c.h_node_ptr, 8 * (size_t)(G + 1));
        std::memcpy(stage + 8 * (G + 1), surv_base.data(), 8 * (size_t)(G + 1));
        std::memcpy(stage + 16 * (G + 1), gd.data(), sizeof(GraphDesc) * (size_t)G);
        if (depths) {
            char* dp = stage + 16 * (G + 1) + sizeof(GraphDesc) * (size_t)G;
            std::memcpy(dp, c.h_depths, 8 * (size_t)(nseg * G));
            std::memcpy(dp + 8 * nseg * G, seg_sb.data(), 8 * seg_sb.size());
        }
        RLAP_HIPCHK(hipMemcpyAsync(W.node_ptr_d.p, stage, host_block_bytes(G, z.D), hipMemcpyHostToDevice, s));
    }
    {
        Fills F;
        F.add(W.scal.p, sizeof(Scalars) / 4, 0);
        if (c.o_v != OV_RANDOM) {   // the bucket stacks and the never-moved lists: PQ orders only
            F.add(W.bs_cnt.p, bucket_total, 0); F.add(W.bs_alloc.p, bucket_total, 0);
            F.add(W.ocur.p, bucket_total, 0); F.add(W.oend.p, bucket_total, 0);
        }
        F.add(W.bs_pool_top.p, 1, 0);
        F.add(W.batch_pos.p, N, -1);
        F.add(W.ext.as<int32_t>() + S0, 1, 0); F.add(W.cnt.as<int32_t>() + S0, 1, 0);
        if (depths) F.add(reinterpret_cast<CallResults*>(W.results.p) + 1, 2 * (nseg * G + 3), 0);   // row pointers of the snapshots, scratch maximum, stop word
        if (G == 1) F.add(W.vgraph.p, N, 0);
        F.launch(s);
    }
    if (G > 1) hipLaunchKernelGGL(k_vertex_graph, dim3(nblk(N, 256)), dim3(256), 0, s, W.node_ptr_d.as<int64_t>(), (int)G, W.vgraph.as<int32_t>(), N);

    const int kbits = (int)bits_for((uint64_t)(N1 > 1 ? N1 - 1 : 1));
    bool swapped = false;   // the input was in (row, col) order and is read transposed (same matrix when it is exactly symmetric)
    uint64_t* keys_sorted = W.keys1.as<uint64_t>();
    uint32_t* idx_sorted = W.idx1.as<uint32_t>();
    uint32_t* rowid = W.idx0.as<uint32_t>();   // dense row ids of the slots (key of the twin sort); a buffer the COO sort has left free
    if (E1eff > 0) {
        hipLaunchKernelGGL(k_edge_keys, dim3(nblk(E1eff, 256)), dim3(256), 0, s, c.d_row, c.d_col, c.d_w, E, N1, G1 > 1 ? W.vgraph.as<int32_t>() : (const int32_t*)nullptr,
                           c.symmetrize, kbits, W.keys0.as<uint64_t>(), W.idx0.as<uint32_t>(), flags);
        // Large inputs: one early look at the order flags (the call's only other host synchronisation) -- a COO that is sorted by
        // (col, row) needs no sort, one sorted by (row, col) (PyG coalesce) is read transposed and needs none either; exact symmetry,
        // which makes the transposed reading the same matrix, is verified with the twins (else the call is repeated with the sort).
        bool skip_sort = false;
        int64_t skip_min = SORT_SKIP_MIN;
        if (const char* e = std::getenv("RLAP_SORT_SKIP_MIN")) skip_min = std::atoll(e);   // (tests: exercise the order check on small inputs)
        if (E1eff >= skip_min && !c.symmetrize && !h->force_sort) {
            int32_t fl[FLAG_COUNT];
            RLAP_HIPCHK(hipMemcpyAsync(fl, flags, sizeof(fl), hipMemcpyDeviceToHost, s));
            RLAP_HIPCHK(hipStreamSynchronize(s));
            if (!fl[FLAG_UNSORTED_CR]) skip_sort = true;
            else if (!fl[FLAG_UNSORTED_RC] && !fl[FLAG_RANGE]) {
                hipLaunchKernelGGL(k_edge_keys, dim3(nblk(E1eff, 256)), dim3(256), 0, s, c.d_col, c.d_row, c.d_w, E, N1, G1 > 1 ? W.vgraph.as<int32_t>() : (const int32_t*)nullptr,
                                   0, kbits, W.keys0.as<uint64_t>(), W.idx0.as<uint32_t>(), flags);
                skip_sort = true; swapped = true;
            }
        }
        st.reserved = skip_sort ? (swapped ? 2 : 1) : 0;
        if (skip_sort) {
            keys_sorted = W.keys0.as<uint64_t>(); idx_sorted = W.idx0.as<uint32_t>();
            rowid = W.idx1.as<uint32_t>();
        } else {
            // keys are (col << kbits | row) with ids < N, or all ones for dropped entries (bit 2 * kbits makes these sort last)
            int rc = sort_pairs(h, ST, W.keys0.as<uint64_t>(), W.keys1.as<uint64_t>(), W.idx0.as<uint32_t>(), W.idx1.as<uint32_t>(), E1eff, 0,
                                (unsigned)std::min(64, 2 * kbits + 1));
            if (rc) return rc;
        }
        { Fills F2; F2.add(rowid, E1eff, (int32_t)N1); F2.launch(s); }   // dense row-id array: slots beyond nnz hold N1 (sorts last)
        hipLaunchKernelGGL(k_heads, dim3(nblk(E1eff + 1, 256)), dim3(256), 0, s, keys_sorted, E1eff, W.head.as<int32_t>());
        int rc = excl_scan(h, ST, W.head.as<int32_t>(), W.pos.as<int32_t>(), E1eff + 1);
        if (rc) return rc;
        hipLaunchKernelGGL(k_fill_csr, dim3(nblk(E1eff, 256)), dim3(256), 0, s, keys_sorted, idx_sorted, W.head.as<int32_t>(),
                           W.pos.as<int32_t>(), c.d_w, E1eff, (c.symmetrize && !c.d_w) ? 1 : 0, kbits, W.ent.as<Slot>(), W.slot_col.as<int32_t>(),
                           reinterpret_cast<int32_t*>(rowid));
    }
    // (nnz = pos[E1eff]: k_colptr reads it there and files it in the scalar block and as the pool's first free slot)
    const int32_t* nnz_src = E1eff > 0 ? W.pos.as<int32_t>() + E1eff : (const int32_t*)&SC->pad;   // (no entries: a zeroed word of its own, not the output word -- both are __restrict__)
    hipLaunchKernelGGL(k_colptr, dim3(nblk(N1 + 1, 256)), dim3(256), 0, s, W.slot_col.as<int32_t>(), nnz_src, (int32_t)N1,
                       W.colptr.as<int32_t>(), nnz_p, W.pool_top.as<int32_t>());
    if (E1eff > 0) {
        // twins: stable sort of the slots by row id (keys0 is free again: sorted keys in its first half, the slot order T in its second)
        uint32_t* skeys = W.keys0.as<uint32_t>();
        uint32_t* T = skeys + Eeff;
        rocprim::counting_iterator<uint32_t> iota(0u);
        size_t bytes = 0;
        RLAP_HIPCHK(rocprim::radix_sort_pairs(nullptr, bytes, rowid, skeys, iota, T, (size_t)E1eff, 0u, (unsigned)std::min(32, kbits + 1), s));
        if (bytes > ST.bytes) return RLAP_E_INTERNAL;
        bytes = ST.bytes;
        RLAP_HIPCHK(rocprim::radix_sort_pairs(ST.p, bytes, rowid, skeys, iota, T, (size_t)E1eff, 0u, (unsigned)std::min(32, kbits + 1), s));
        hipLaunchKernelGGL(k_twin_sorted, dim3((unsigned)std::min<int64_t>(nblk(E1eff, 256), 4096)), dim3(256), 0, s, W.ent.as<Slot>(), T, nnz_p, acc);
        hipLaunchKernelGGL(k_twin_store, dim3((unsigned)std::min<int64_t>(nblk(E1eff, 256), 4096)), dim3(256), 0, s, W.ent.as<Slot>(), T, nnz_p);
    }
    if (K > 1)   // the union's CSR: copy k of every slot, column start and slot column, shifted by k * nnz / k * N1 (nnz read on the device)
        hipLaunchKernelGGL(k_views_replicate, dim3((unsigned)std::min<int64_t>(nblk(E1eff, 256), 2048)), dim3(256), 0, s, W.ent.as<Slot>(),
                           W.slot_col.as<int32_t>(), W.colptr.as<int32_t>(), nnz_src, (int32_t)N1, (int32_t)K, nnz_p, W.pool_top.as<int32_t>());
    // per-graph scratch of the long-column fall-backs (needs the per-graph nnz: filled on the device)
    hipLaunchKernelGGL(k_gd_scratch, dim3(1), dim3(256), 0, s, W.colptr.as<int32_t>(), W.node_ptr_d.as<int64_t>(), (int32_t)G, W.gd_d.as<GraphDesc>());

    // ---------------- PQ init ----------------
    const unsigned gbits = bits_for((uint64_t)(G > 0 ? G - 1 : 0));
    hipLaunchKernelGGL(k_pq_init, dim3(nblk(N, 256)), dim3(256), 0, s, W.colptr.as<int32_t>(), W.vgraph.as<int32_t>(), (int32_t)N, W.vrec.as<VRec>(),
                       W.skey0.as<uint64_t>(), W.sval0.as<uint32_t>());
    if (c.o_v != OV_RANDOM) {   // (o_v = random has no queue: k_pq_init's vertex records are all it needs)
        // key = graph << 32 | degree: only the bits that can be set take part in the sort
        int rc = sort_pairs(h, ST, W.skey0.as<uint64_t>(), W.skey1.as<uint64_t>(), W.sval0.as<uint32_t>(), W.orig_order.as<uint32_t>(), N, 0, 32 + gbits);
        if (rc) return rc;
        hipLaunchKernelGGL(k_bucket_bounds, dim3(nblk(N, 256)), dim3(256), 0, s, W.orig_order.as<uint32_t>(), W.vrec.as<VRec>(), W.vgraph.as<int32_t>(),
                           W.gd_d.as<GraphDesc>(), (int32_t)N, W.ocur.as<int32_t>(), W.oend.as<int32_t>(), W.origpos.as<int32_t>());
    }

    // ---------------- o_v = random: the node_id vector ----------------
    const int64_t* d_perm = c.d_perm;
    if (c.o_v == OV_RANDOM) {
        if (!d_perm) {
            hipLaunchKernelGGL(k_perm_keys, dim3(nblk(N, 256)), dim3(256), 0, s, W.vgraph.as<int32_t>(), W.gd_d.as<GraphDesc>(), (int32_t)N, c.seed,
                               G > 1 ? (int)gbits : 0, W.skey0.as<uint64_t>(), W.sval0.as<uint32_t>());
            int rc = sort_pairs(h, ST, W.skey0.as<uint64_t>(), W.skey1.as<uint64_t>(), W.sval0.as<uint32_t>(), W.sval1.as<uint32_t>(), N, 0, 64);
            if (rc) return rc;
            hipLaunchKernelGGL(k_widen_u32, dim3(nblk(N, 256)), dim3(256), 0, s, W.sval1.as<uint32_t>(), (int32_t)N, W.genperm.as<int64_t>());
            d_perm = W.genperm.as<int64_t>();
        } else {
            RLAP_HIPCHK(hipMemsetAsync(W.permchk.p, 0, 4 * N, s));
            hipLaunchKernelGGL(k_perm_check, dim3(nblk(N, 256)), dim3(256), 0, s, d_perm, W.vgraph.as<int32_t>(), W.gd_d.as<GraphDesc>(), (int32_t)N,
                               W.permchk.as<int32_t>(), flags);
        }
    }

    Arrays A;
    A.colptr = W.colptr.as<int32_t>();
    A.e = W.ent.as<Slot>();
    A.slot_cap = (int32_t)slot_cap; A.pool_top = W.pool_top.as<int32_t>();
    A.vr = W.vrec.as<VRec>();
    A.ocur = W.ocur.as<int32_t>(); A.oend = W.oend.as<int32_t>();
    A.orig_order = W.orig_order.as<int32_t>();
    A.bs_cnt = W.bs_cnt.as<int32_t>(); A.bs_alloc = W.bs_alloc.as<int32_t>(); A.bs_dir = W.bs_dir.as<int32_t>();
    A.bs_v = W.bs_v.as<int32_t>(); A.bs_id = W.bs_id.as<int32_t>();
    A.bs_pool_top = W.bs_pool_top.as<int32_t>(); A.bs_pool_cap = (int32_t)log_total;
    A.rng = h->rng_ptr; A.rng_len = rng_len_eff;
    A.perm = d_perm; A.o_v = c.o_v; A.o_n = c.o_n; A.shuffle_seed = c.seed;
    A.rng_mode = h->rng_mode ? RNG_COUNTER : RNG_STREAM; A.vbase = 0;
    if (A.rng_mode == RNG_COUNTER) A.rng_len = (int64_t)1 << 62;   // (no table is read: the stream-length checks of the kernels never fire)
    ElimScratch ES;
    ES.rec = W.scr_rec.as<SRec>(); ES.i32 = W.scr_i32.as<int32_t>(); ES.f64 = W.scr_f64.as<double>(); ES.cap = scr_total;
    ES.eqtab = h->eqtab.as<uint8_t>();
    ES.prof = nullptr;
    const char* prof_env = std::getenv("RLAP_PHASE_PROFILE");   // diagnostic only: per-phase clock sums of graph 0
    if (prof_env && prof_env[0] == '1' && h->prof.p) {
        RLAP_HIPCHK(hipMemsetAsync(h->prof.p, 0, 8 * 80, s));
        ES.prof = h->prof.as<long long>();
    }
    ES.poison = h->poison;
    ES.jitter = h->jitter;
    ES.narrow_batch = NARROW_BATCH;
    if (const char* e = std::getenv("RLAP_NARROW_BATCH")) ES.narrow_batch = std::min(256, std::max(1, std::atoi(e)));   // diagnostic override

    if (h->timing) RLAP_HIPCHK(hipEventRecord(h->ev[1], s));
    // ---------------- elimination ----------------
    // 128-slot candidates for o_v = random when the columns run long: 12 or more entries per vertex on average (from the input
    // sizes: no read-back).  Measured (ms per call, 64 -> 128 slots): BA(1M,10) 2950 -> 2180, BA(169343,7) 260 -> 248, BA(4096,8)
    // 10.2 -> 9.2; BA(20000,5) 23.0 -> 23.4 and sparser graphs lose (their rounds fill 64 candidates and get only 32)
    const bool wide = c.o_v == OV_RANDOM && nnz_ub >= 12 * N && N >= 512;
    FlowArrays FA;
    std::memset(&FA, 0, sizeof(FA));
    FlowParams FP;
    std::memset(&FP, 0, sizeof(FP));
    int shape = 1;
    unsigned grid = 0;
    GraphDesc* gd_d = W.gd_d.as<GraphDesc>();
    if (flow) {
        // dataflow elimination (rlap_flow.hip): every position of the order is one wave's, on any compute unit
        FA.cdir = W.f_cdir.as<int32_t>(); FA.atag = W.f_atag.as<int32_t>(); FA.lb = W.f_lb.as<unsigned long long>();
        FA.qv = W.f_qv.as<int32_t>(); FA.qg = W.f_qg.as<int32_t>(); FA.ctrl = W.f_ctrl.as<int32_t>(); FA.Q = (int32_t)z.flow_Q;
        FP.vgraph = W.vgraph.as<int32_t>(); FP.gd = gd_d; FP.in_flags = flags; FP.in_acc = acc;
        FP.scr = W.f_scr.as<char>(); FP.scr_entries = (int32_t)z.flow_scr;
        FP.spin_limit = 4000; FP.jitter = h->jitter; FP.poison = h->poison;
        FP.prof = ES.prof;
        FP.trace = nullptr;
        const char* trace_env = std::getenv("RLAP_FLOW_TRACE");   // diagnostic only: per-position time stamps, written to the named file after the call
        if (trace_env && trace_env[0]) {
            ENSURE(h->trace, (size_t)z.flow_Q * 48);
            RLAP_HIPCHK(hipMemsetAsync(h->trace.p, 0, (size_t)z.flow_Q * 48, s));
            FP.trace = h->trace.as<long long>();
        }
        if (const char* e = std::getenv("RLAP_FLOW_STALL_MS")) FP.spin_limit = std::max(1, std::atoi(e));
        RLAP_HIPCHK(hipMemsetAsync(W.f_ctrl.p, 0, FC_WORDS * 4, s));
        FA.qorder = nullptr; FA.Qclaim = FA.Q;
        const bool interleave = G > 1 && nelim_total > 0;   // a batch: claims run over the graphs' positions interleaved, so that every graph has waves
        launch_flow_setup(s, A, FA, FP, W.slot_col.as<int32_t>(), nnz_p, (int32_t)N, Eeff, interleave ? W.skey0.as<uint64_t>() : nullptr,
                          interleave ? W.sval0.as<uint32_t>() : nullptr, (int)gbits);
        if (interleave) {
            int rc = sort_pairs(h, ST, W.skey0.as<uint64_t>(), W.skey1.as<uint64_t>(), W.sval0.as<uint32_t>(), W.sval1.as<uint32_t>(), nelim_total, 0, std::min(64u, 32u + gbits));
            if (rc) return rc;
            FA.qorder = W.sval1.as<uint32_t>(); FA.Qclaim = (int32_t)nelim_total;
            if (depths && nseg > 1) {
                // segments as contiguous claim ranges (stable regrouping by segment), in sval0: the output pass of every snapshot
                // writes its order into sval1, and o_v = random leaves sval0 alone from here on
                hipLaunchKernelGGL(k_flow_seg_keys, dim3(nblk(nelim_total, 256)), dim3(256), 0, s, W.sval1.as<uint32_t>(), (int32_t)nelim_total, FA.qg, gd_d,
                                   W.depth_t.as<int64_t>(), (int32_t)nseg, (int32_t)G, W.skey0.as<uint64_t>());
                rc = sort_pairs(h, ST, W.skey0.as<uint64_t>(), W.skey1.as<uint64_t>(), W.sval1.as<uint32_t>(), W.sval0.as<uint32_t>(), nelim_total, 0,
                                bits_for((uint64_t)(nseg - 1)));
                if (rc) return rc;
                FA.qorder = W.sval0.as<uint32_t>();
            }
        }
        shape = G >= 48 ? 3 : 1;   // 1: 76 KB of LDS, two workgroups per CU, four waves each (three help with long sorts); 4: the same with one wave; 3: 40 KB, four; 2: 17 KB, eight
        if (const char* e = std::getenv("RLAP_FLOW_SHAPE")) { if (e[0] >= '1' && e[0] <= '4') shape = e[0] - '0'; }   // diagnostic override
        grid = (shape == 2 ? 8u : shape == 3 ? 4u : 2u) * (unsigned)h->n_cu;   // (workgroups: one position each)
        if (const char* e = std::getenv("RLAP_FLOW_WAVES")) grid = (unsigned)std::max(1, std::atoi(e));
    }
    CallResults* res_d = W.results.as<CallResults>();
    int64_t* out_ptr_d = reinterpret_cast<int64_t*>(res_d + 1);
    unsigned long long* scr_max_d = reinterpret_cast<unsigned long long*>(out_ptr_d + nseg * G + 1);   // (depths call only)
    int32_t* stop_d = depths ? reinterpret_cast<int32_t*>(scr_max_d + 1) : nullptr;                    // (depths call only: k_depth_stop)
    ScScratch SS;
    SS.rec = W.sc_rec.as<SRec>(); SS.i32 = W.sc_i32.as<int32_t>(); SS.f64 = W.sc_f64.as<double>(); SS.cap = scr_budget; SS.top = counters + 0; SS.flags = flags;
    // One segment for the other calls.  A depths call runs the elimination in segments [ne[k-1][j], ne[k][j]) of every graph j, each
    // followed by the output pass of its snapshot: the state a segment stops in is the state the next one starts from.
    for (int64_t seg = 0; seg < nseg; ++seg) {
        const int64_t Q_lo = seg > 0 ? seg_Q[(size_t)seg - 1] : 0, Q_hi = seg_Q[(size_t)seg];
        const int64_t Sk = depths ? N - Q_hi : S;
        const bool last = seg + 1 == nseg;
        const bool run_seg = seg == 0 || Q_hi > Q_lo;   // (no graph advances: the state is already the snapshot's)
        if (depths && run_seg)
            hipLaunchKernelGGL(k_depth_set, dim3(nblk(G, 256)), dim3(256), 0, s, gd_d, W.depth_t.as<int64_t>() + seg * G, (int32_t)G, flow ? 1 : 0,
                               seg > 0 ? 1 : 0);
        if (run_seg) {
            if (flow) {
                if (depths) {
                    // claims of the segment: with a claim order (batches), its range [Q_{k-1}, Q_k) of it; without (one graph), look-back
                    // indices p + 1 (graph 0's sentinel first)
                    const int64_t off = FA.qorder ? 0 : 1;
                    FA.Qclaim = (int32_t)(Q_hi + off);
                    if (seg > 0) launch_flow_segment(s, FA, (int32_t)(Q_lo + off), stop_d);
                }
                launch_flow_eliminate(shape, grid, s, A, FA, FP);
                launch_flow_finish(s, A, FA, gd_d, (int32_t)N, (int32_t)G);
            } else {
                // (squeeze passes: the elimination ends in whichever arena its last pass wrote -- A names that one from here on)
                SqueezeBufs SQ;
                SQ.passes = squeeze; SQ.e2 = W.sq_ent.as<Slot>(); SQ.colptr2 = W.sq_colptr.as<int32_t>(); SQ.rank = W.sq_rank.as<int32_t>();
                SQ.cnt = W.sq_cnt.as<int32_t>(); SQ.longlist = W.sq_list.as<int32_t>(); SQ.nlong = W.sq_nlong.as<int32_t>();
                SQ.marks = W.sq_marks.as<int32_t>(); SQ.vgraph = W.vgraph.as<int32_t>(); SQ.scan_tmp = W.sorttmp.p; SQ.scan_tmp_bytes = z.sort_tmp;
                SQ.N = (int32_t)N;
                Arrays A_end;
                RLAP_HIPCHK((hipError_t)launch_eliminate_batch(c.o_v, c.o_n, (unsigned)G, h->n_cu, s, A, gd_d, ES, W.batch_pos.as<int32_t>(), flags, acc, wide,
                                                               squeeze > 0 ? &SQ : nullptr, &A_end));
                A = A_end;
            }
            RLAP_HIPCHK(hipGetLastError());
            if (depths) hipLaunchKernelGGL(k_depth_stop, dim3(1), dim3(256), 0, s, gd_d, (int32_t)G, stop_d);
        }
        if (h->timing) RLAP_HIPCHK(hipEventRecord(h->ev[2], s));

        // ---------------- output ----------------
        uint32_t* order = nullptr;
        bool permuted = false;   // the dataflow kernel's surviving columns were put into tag order in place
        const int32_t ro_cap = (int32_t)(h->dbg_ro_cap >= 0 ? std::max<int64_t>(1, std::min<int64_t>(h->dbg_ro_cap, Eeff)) : Eeff);   // (test hook: smaller)
        uint32_t* home = reinterpret_cast<uint32_t*>(W.head.p);
        if (c.o_v == OV_RANDOM) {
            hipLaunchKernelGGL(k_sc_perm_order, dim3(nblk(N, 256)), dim3(256), 0, s, d_perm, W.vgraph.as<int32_t>(), gd_d,
                               depths ? W.depth_sb.as<int64_t>() + seg * (G + 1) : W.surv_base_d.as<int64_t>(), (int32_t)N, W.sval1.as<uint32_t>());
            order = W.sval1.as<uint32_t>();
            if (flow && Sk > 0 && Eeff > 0) {
                // tag order of the surviving columns: concurrent eliminations pushed into them out of order (rlap_flow.h)
                launch_flow_ro_count(s, A, FA, order, (int32_t)Sk, W.f_rocnt.as<int32_t>());
                { int rc = excl_scan(h, ST, W.f_rocnt.as<int32_t>(), W.f_rooff.as<int32_t>(), Sk + 1); if (rc) return rc; }
                launch_flow_ro_emit(s, A, FA, order, (int32_t)Sk, W.f_rooff.as<int32_t>(), W.keys0.as<uint64_t>(), W.idx0.as<uint32_t>(), home, ro_cap, &gd_d[0].status);
                const unsigned kb = bits_for((uint64_t)std::max<int64_t>(Sk - 1, 1)) + 32u;
                { int rc = sort_pairs(h, ST, W.keys0.as<uint64_t>(), W.keys1.as<uint64_t>(), W.idx0.as<uint32_t>(), W.idx1.as<uint32_t>(), ro_cap, 0, std::min(64u, kb)); if (rc) return rc; }
                launch_flow_ro_permute(s, A, FA, W.f_rooff.as<int32_t>(), (int32_t)Sk, W.idx1.as<uint32_t>(), W.keys1.as<uint64_t>(), home, ro_cap, reinterpret_cast<Slot*>(W.tmp_val.p));
                RLAP_HIPCHK(hipGetLastError());
                permuted = true;
            }
        } else {
            hipLaunchKernelGGL(k_sc_keys, dim3(nblk(N, 256)), dim3(256), 0, s, W.vrec.as<VRec>(), W.origpos.as<int32_t>(),
                               W.vgraph.as<int32_t>(), gd_d, (int32_t)N, W.skey0.as<uint64_t>(), W.sval0.as<uint32_t>());
            // key = bucket << 32 | order, all ones for eliminated vertices
            int rc = sort_pairs(h, ST, W.skey0.as<uint64_t>(), W.skey1.as<uint64_t>(), W.sval0.as<uint32_t>(), W.sval1.as<uint32_t>(), N, 0, 64);
            if (rc) return rc;
            order = W.sval1.as<uint32_t>();
        }
        if (Sk > 0)
            hipLaunchKernelGGL(k_sc_ext, dim3(nblk(Sk, 256)), dim3(256), 0, s, order, A.colptr, W.vrec.as<VRec>(), (int32_t)Sk, flags, acc, W.ext.as<int32_t>(), stop_d);
        { int rc = excl_scan(h, ST, W.ext.as<int32_t>(), W.tmp_off.as<int64_t>(), Sk + 1); if (rc) return rc; }
        if (h->timing) RLAP_HIPCHK(hipEventRecord(h->ev[3], s));
        if (Sk > 0) {
            int32_t* tiercounts = reinterpret_cast<int32_t*>(counters + 4);   // 8 ints: tiers 0..7
            if (!h->big_attr_set) {
                RLAP_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sc_merge_big), hipFuncAttributeMaxDynamicSharedMemorySize, BIG_LDS_BYTES));
                RLAP_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sc_merge_mw<8>), hipFuncAttributeMaxDynamicSharedMemorySize, MW_BIG_LDS_BYTES));
                RLAP_HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_sc_merge_mw<4>), hipFuncAttributeMaxDynamicSharedMemorySize, MW_MID_LDS_BYTES));
                h->big_attr_set = true;
            }
            ScLaunch X;
            X.main = s; X.side[0] = h->side[0]; X.side[1] = h->side[1];
            for (int q = 0; q < 3; ++q) X.ev[q] = h->fork_ev[q];
            launch_sc_merge(X, A, gd_d, W.vgraph.as<int32_t>(), order, W.ext.as<int32_t>(), W.tmp_off.as<int64_t>(), (int32_t)Sk,
                            W.tmp_nbr.as<int32_t>(), W.tmp_val.as<double>(), W.cnt.as<int32_t>(), SS, live, W.biglist.as<int32_t>(), tiercounts,
                            W.hugelists.as<uint16_t>());
            RLAP_HIPCHK(hipGetLastError());
        }
        if (h->timing) RLAP_HIPCHK(hipEventRecord(h->ev[4], s));
        { int rc = excl_scan(h, ST, W.cnt.as<int32_t>(), W.row_off.as<int64_t>(), Sk + 1); if (rc) return rc; }
        if (h->timing) RLAP_HIPCHK(hipEventRecord(h->ev[5], s));
        if (Sk > 0 && c.out_cap > 0) {
            const int64_t rows_ub = std::min<int64_t>(c.out_cap, slot_cap);
            unsigned cgrid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((rows_ub + 255) / 256, 256 * 8));
            hipLaunchKernelGGL(k_sc_compact, dim3(cgrid), dim3(256), 0, s, order, W.cnt.as<int32_t>(), W.row_off.as<int64_t>(), W.tmp_off.as<int64_t>(),
                               W.tmp_nbr.as<int32_t>(), W.tmp_val.as<double>(), (int32_t)Sk, c.d_out, c.out_cap, K > 1 ? (int32_t)N1 : 0,
                               depths ? (const int64_t*)(out_ptr_d + seg * G) : (const int64_t*)nullptr);
            RLAP_HIPCHK(hipGetLastError());
        }
        if (depths) {
            // the next segment continues from the elimination's own state: the tag-order permutation is undone (the same kernels with
            // source and destination swapped; home, the sorted slots and their tags are buffers the output pass leaves alone, and the
            // staging copy is free again), so that every twin link points where it did
            if (permuted && !last) {
                launch_flow_ro_permute(s, A, FA, W.f_rooff.as<int32_t>(), (int32_t)Sk, home, W.keys1.as<uint64_t>(), W.idx1.as<uint32_t>(), ro_cap, reinterpret_cast<Slot*>(W.tmp_val.p));
                RLAP_HIPCHK(hipGetLastError());
            }
            hipLaunchKernelGGL(k_depth_close, dim3(1), dim3(256), 0, s, W.row_off.as<int64_t>(), W.depth_sb.as<int64_t>() + seg * (G + 1), (int32_t)G,
                               out_ptr_d + seg * G, counters, live, scr_max_d, last ? -1 : (int32_t)(N - seg_Q[(size_t)seg + 1]), W.ext.as<int32_t>(),
                               W.cnt.as<int32_t>());
            RLAP_HIPCHK(hipGetLastError());
        }
        if (h->timing) RLAP_HIPCHK(hipEventRecord(h->ev[6], s));
    }
    // ---------------- the one read-back ----------------
    if (!depths)
        hipLaunchKernelGGL(k_graph_rows, dim3(nblk(G + 1, 256)), dim3(256), 0, s, W.surv_base_d.as<int64_t>(), W.row_off.as<int64_t>(), (int32_t)G, out_ptr_d);
    hipLaunchKernelGGL(k_collect, dim3(1), dim3(256), 0, s, flags, acc, nnz_p, counters, live, W.tmp_off.as<int64_t>(), W.row_off.as<int64_t>(), (int32_t)S,
                       W.gd_d.as<GraphDesc>(), (int32_t)G, W.pool_top.as<int32_t>(), W.bs_pool_top.as<int32_t>(), flow ? W.f_ctrl.as<int32_t>() + FC_REASON : nullptr,
                       W.sq_marks.as<int32_t>(), (int32_t)squeeze, res_d);
    RLAP_HIPCHK(hipMemcpyAsync(h->h_results, W.results.p, res_bytes, hipMemcpyDeviceToHost, s));
    if (h->timing) RLAP_HIPCHK(hipEventRecord(h->ev[7], s));
    RLAP_HIPCHK(hipStreamSynchronize(s));
    const CallResults& R = *reinterpret_cast<const CallResults*>(h->h_results);
    const int64_t* out_ptr_h = reinterpret_cast<const int64_t*>(reinterpret_cast<const CallResults*>(h->h_results) + 1);

    if (flow) if (const char* trace_env = std::getenv("RLAP_FLOW_TRACE")) if (trace_env[0] && h->trace.p) {
        std::vector<long long> tr((size_t)z.flow_Q * 6);
        RLAP_HIPCHK(hipMemcpy(tr.data(), h->trace.p, tr.size() * 8, hipMemcpyDeviceToHost));
        if (FILE* f = std::fopen(trace_env, "wb")) { std::fwrite(tr.data(), 8, tr.size(), f); std::fclose(f); }
    }
    if (ES.prof && flow) {
        long long pr[40];
        RLAP_HIPCHK(hipMemcpy(pr, h->prof.p, sizeof(pr), hipMemcpyDeviceToHost));
        const char* names[11] = {"claim + wait for pend == 0", "gather", "sort by id (+ tag order)", "merge + publish", "o_n order", "cumsum + recurrence", "look-back wait", "sample", "commit (claims, chunks, stores)", "drain", "decrements"};
        std::fprintf(stderr, "[rlap flow profile] positions=%lld mean live=%.1f mean extent=%.1f; sums over all waves, us per position\n", pr[16], pr[16] ? (double)pr[17] / pr[16] : 0.0, pr[16] ? (double)pr[18] / pr[16] : 0.0);
        for (int k = 0; k < 11; ++k) std::fprintf(stderr, "  %-34s %10.3f ms total  %8.2f us/pos\n", names[k], pr[k] / 1e5, pr[16] ? pr[k] / 100.0 / (double)pr[16] : 0.0);
        if (pr[12] || pr[15]) std::fprintf(stderr, "[rlap flow] RLAP_FLOW_MW_SORT build: %lld sorted index sets out of range; lanes affected with the prepared address %llx, with a fresh one %llx\n", pr[15], pr[13], pr[14]);
        std::fprintf(stderr, "  long columns: %lld (mean live %.0f, max %lld; %lld beyond 900, %lld beyond 1888, %lld beyond 3320 taking %.3f of %.3f ms)\n", pr[36], pr[36] ? (double)pr[37] / pr[36] : 0.0, pr[35], pr[38], pr[39], pr[32], pr[33] / 1e5, pr[34] / 1e5);
        for (int k = 1; k < 11; ++k) std::fprintf(stderr, "    %-32s %10.3f ms total  %8.2f us/col\n", names[k], pr[20 + k] / 1e5, pr[36] ? pr[20 + k] / 100.0 / (double)pr[36] : 0.0);
    } else if (ES.prof) {
        long long pr2[80];
        RLAP_HIPCHK(hipMemcpy(pr2, h->prof.p, sizeof(pr2), hipMemcpyDeviceToHost));
        // two blocks: the 32/64/128-slot round kernel, then the 16-slot one of the degree order (printed first: it runs first)
        for (int blk = 1; blk >= 0; --blk) {
        const long long* pr = pr2 + 40 * blk;
        if (blk == 1 && pr[21] == 0) continue;
        if (blk == 1) std::fprintf(stderr, "[rlap phase profile] 16-slot round kernel:\n");
        else if (pr2[40 + 21] != 0) std::fprintf(stderr, "[rlap phase profile] 32-slot round kernel behind it:\n");
        const char* names[20] = {"P0 select", "P1 permute + closing barrier", "P1b multi-edge cut + P2 offsets", "P3 sample", "P4 replay", "single path", "P5b slots + shared targets", "move order", "pushes", "P1 meta + loads + dependence", "P5a cursors + pool", "P5c rewire stores", "P1 id rank", "P1 (sync)", "P1 o_n order (sorts)", "P1 write pass", "P1 (sync)", "P1 o_n rank", "empty (cost of one stamp)", "P3b dependent candidates (patch)"};
        std::fprintf(stderr, "[rlap phase profile] rounds=%lld singles=%lld (100 MHz ticks); shader clock over the kernel: %.0f MHz\n", pr[22], pr[23], pr[21] > 0 ? 100.0 * (double)pr[20] / (double)pr[21] : 0.0);
        for (int k = 0; k < 20; ++k) std::fprintf(stderr, "  %-22s %10.3f ms\n", names[k], pr[k] / 1e5);
        const char* wnames[9] = {"gather", "sort by id", "merge", "meta loads + order", "cumsum + recurrence", "sample", "replay + slots", "rewire", "pq commit"};
        for (int k = 0; k < 9; ++k) std::fprintf(stderr, "  single/wave: %-20s %10.3f ms\n", wnames[k], pr[24 + k] / 1e5);
        const char* xnames[5] = {"P4.1 hash insert + key loads", "P4.2 replay (uncontended)", "P4.3 sort of the contended records", "P4.4 contended walk", "P5b uncontended slots (rest of P5b = contended walk)"};
        for (int k = 0; k < 5; ++k) std::fprintf(stderr, "  detail: %-52s %10.3f ms\n", xnames[k], pr[33 + k] / 1e5);
        }
    }

    st.nnz = R.nnz;
    st.n_draws = R.n_draws;
    st.n_rounds = R.rounds; st.n_singles = R.singles; st.n_rounds_narrow = R.rounds_narrow;
    st.n_squeezes = R.n_squeezes;
    const int64_t m_total = depths ? out_ptr_h[nseg * G] : R.m_total;   // (depths: the rows of all snapshots)
    st.out_rows = m_total;
    st.live_entries = R.live_total;
    if (flow && R.status == ST_INTERNAL) *flow_abort = R.flow_abort;
    if (h->timing) {
        float t = 0;
        (void)hipEventElapsedTime(&t, h->ev[0], h->ev[1]); st.ms_setup = t;
        (void)hipEventElapsedTime(&t, h->ev[1], h->ev[2]); st.ms_elim = t;
        (void)hipEventElapsedTime(&t, h->ev[2], h->ev[7]); st.ms_output = t;
        (void)hipEventElapsedTime(&t, h->ev[3], h->ev[4]); st.ms_sc_merge = t;
        (void)hipEventElapsedTime(&t, h->ev[5], h->ev[6]); st.ms_sc_compact = t;
        (void)hipEventElapsedTime(&t, h->ev[0], h->ev[7]); st.ms_total = t;
    }
    if (c.st) *c.st = st;
    // input errors first (the elimination was skipped), then growth limits (the call is repeated), then the output size
    if (R.status == ST_INDEX_RANGE || R.flags[FLAG_RANGE]) return RLAP_E_INDEX_RANGE;
    if (R.status == ST_BAD_ARG || R.flags[FLAG_CROSS] || R.flags[FLAG_PERM]) return RLAP_E_BAD_ARG;
    if (R.status == ST_NOT_SYMMETRIC) return RLAP_E_NOT_SYMMETRIC;
    if (R.status) {
        if (R.status == ST_POOL_OVERFLOW) *retry_kind = 1;
        else if (R.status == ST_LOG_OVERFLOW) *retry_kind = 2;
        else if (R.status == ST_RNG_OVERFLOW) *retry_kind = 3;
        else if (R.status == ST_FLOW_SCRATCH) *retry_kind = 6;
        else if (R.status == ST_FLOW_REORDER) *retry_kind = 7;
        else if (R.status == ST_INTERNAL && flow) *retry_kind = 8;   // the dataflow kernel gave up (stall watchdog, index check, ...: *flow_abort): once more on the round kernel
        return R.status;
    }
    if (R.flags[FLAG_SCR]) { *retry_kind = 4; *retry_need = R.scr_need; return RLAP_E_INTERNAL; }
    if (swapped && R.acc[0] != 0.0) { *retry_kind = 5; return RLAP_E_INTERNAL; }   // symmetric only within the tolerance: repeat, reading the input as given
    const int64_t nptr = depths ? nseg * G : G;
    for (int64_t g = 0; g <= nptr; ++g) c.h_out_row_ptr[g] = out_ptr_h[g];
    if (m_total > c.out_cap) { c.h_out_row_ptr[nptr] = m_total; return RLAP_E_OUT_OVERFLOW; }
    return RLAP_OK;
}

struct DeviceGuard {
    int prev = -1; bool changed = false;
    explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess); }
    ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};

int run_call(rlap_handle h, const Call& c) {
    std::lock_guard<std::mutex> lock(h->mu);
    DeviceGuard dg(h->device);
    int rc = RLAP_E_INTERNAL;
    int retries = 0;
    int32_t causes = 0, abort_reason = 0;   // (rlap_stats.retry_causes / flow_abort)
    for (int attempt = 0; attempt < 10; ++attempt) {
        int kind = 0; int64_t need = 0; int32_t fa = 0;
        rc = run_once(h, c, &kind, &need, &fa);
        h->dbg_ro_cap = -1;   // (test hook: the first attempt only)
        if (fa) abort_reason = fa;
        if (kind == 0) break;
        causes |= 1 << kind;
        ++retries;
        // a test hook's tiny limit applies to the first attempt only; afterwards the regular growth takes over
        if (kind == 1) { if (h->dbg_pool >= 0) h->dbg_pool = -1.0; else h->pool_factor = h->pool_factor * 2 + 1; }
        else if (kind == 2) { if (h->dbg_log >= 0) h->dbg_log = -1.0; else h->log_factor *= 2; }
        else if (kind == 3) { if (h->dbg_rng >= 0) h->dbg_rng = -1; else h->rng_min = std::max<int64_t>(2 * h->rng_len, 1 << 16); }
        else if (kind == 4) { if (h->dbg_scr >= 0) h->dbg_scr = -1; h->scr_budget = std::max<int64_t>(h->scr_budget, need + 8); }
        else if (kind == 5) h->force_sort = true;
        else if (kind == 6) { if (h->dbg_scr >= 0) h->dbg_scr = -1; else h->flow_scr_factor *= 4; }
        else if (kind == 7 || kind == 8) h->flow_off_once = true;
    }
    h->force_sort = false; h->flow_off_once = false;
    h->total_retries += retries;
    if (c.st) { c.st->n_retries = retries; c.st->retry_causes = causes; c.st->flow_abort = abort_reason; }
    return rc;
}

// One elimination as the exports ask for it: K views (1: one) of a batch of G graphs given by the caller's h_node_ptr[G+1], with D
// nested depths each (0: not a depths call) from h_num_remove[max(D, 1)][K*G].
struct Request {
    const int64_t* d_row = nullptr; const int64_t* d_col = nullptr; const double* d_w = nullptr; int64_t E = 0;
    int64_t G = 1; const int64_t* h_node_ptr = nullptr; int64_t K = 1, D = 0; const int64_t* h_num_remove = nullptr;
    int o_v = 0, o_n = 0; const int64_t* d_perm = nullptr; uint64_t seed = 0;
    double* d_out = nullptr; int64_t out_cap = 0; int64_t* h_out_ptr = nullptr; int symmetrize = 0; rlap_stats* st = nullptr;
};

// Every argument check of the exports, in this order: null pointers and counts, o_v / o_n, the COO, the output, node_ptr (starts
// at 0, never decreases), the size limits of a batched call on the K-fold union (K*G and K*N below 2^30, K*E below 2^31; D*K*G
// below 2^30), the depth columns (never decrease).  Then the call runs on the union.
int eliminate(rlap_handle h, const Request& r) {
    const int64_t E = r.E, G = r.G, K = r.K, D = r.D;
    if (!h || E < 0 || G < 1 || K < 1 || D < 0 || !r.h_node_ptr || !r.h_num_remove || !r.h_out_ptr) return RLAP_E_BAD_ARG;
    if (r.o_v < 0 || r.o_v > 2 || r.o_n < 0 || r.o_n > 2) return RLAP_E_BAD_ARG;
    if (E > 0 && (!r.d_row || !r.d_col)) return RLAP_E_BAD_ARG;
    if (r.out_cap > 0 && !r.d_out) return RLAP_E_BAD_ARG;
    if (r.h_node_ptr[0] != 0) return RLAP_E_BAD_ARG;
    for (int64_t g = 0; g < G; ++g) if (r.h_node_ptr[g + 1] < r.h_node_ptr[g]) return RLAP_E_BAD_ARG;
    const int64_t N = r.h_node_ptr[G], L30 = (int64_t)1 << 30, L31 = (int64_t)1 << 31;
    if (K >= L30 || G >= L30 || K * G >= L30 || N > (L30 - 1) / K || E > (L31 - 1) / K) return RLAP_E_TOO_LARGE;
    const int64_t P = K * G;
    if (D > 0 && D >= L30 / P) return RLAP_E_TOO_LARGE;
    for (int64_t d = 1; d < D; ++d)
        for (int64_t j = 0; j < P; ++j) if (r.h_num_remove[d * P + j] < r.h_num_remove[(d - 1) * P + j]) return RLAP_E_BAD_ARG;
    // graph k * G + g of the union: ids [k * N + node_ptr[g], k * N + node_ptr[g + 1]); depth d of it is h_num_remove[d][k * G + g]
    std::vector<int64_t> np((size_t)(P + 1));
    for (int64_t k = 0; k < K; ++k)
        for (int64_t g = 0; g < G; ++g) np[(size_t)(k * G + g)] = k * N + r.h_node_ptr[g];
    np[(size_t)P] = K * N;
    const Call c{.d_row = r.d_row, .d_col = r.d_col, .d_w = r.d_w, .E = E, .G = P, .h_node_ptr = np.data(),
                 .h_t = r.h_num_remove + (D > 0 ? D - 1 : 0) * P, .o_v = r.o_v, .o_n = r.o_n, .d_perm = r.d_perm, .seed = r.seed,
                 .d_out = r.d_out, .out_cap = r.out_cap, .h_out_row_ptr = r.h_out_ptr, .st = r.st, .symmetrize = r.symmetrize,
                 .K = K, .h_depths = D > 0 ? r.h_num_remove : nullptr, .D = D};
    return run_call(h, c);
}

}  // namespace

extern "C" {

// the body of rlap_create: any failure leaves a partly built handle that rlap_create hands to rlap_destroy
static int create_into(rlap_handle h) {
    for (auto& e : h->ev) RLAP_HIPCHK(hipEventCreate(&e));
    for (auto& e : h->fork_ev) RLAP_HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& st : h->side) RLAP_HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    // everything a call needs besides its arena and the uniform table is allocated here, once: the equal-key permutation tables
    // (built on one of the handle's own non-blocking streams -- not the null stream, which would serialise against every blocking
    // stream of the caller -- and finished before rlap_create returns), the pinned read-back block, the diagnostic profile
    ENSURE(h->small, 256);
    ENSURE(h->eqtab, EQTAB_BYTES);
    launch_eq_tables(h->side[0], h->eqtab.as<uint8_t>());
    RLAP_HIPCHK(hipGetLastError());
    RLAP_HIPCHK(hipStreamSynchronize(h->side[0]));
    RLAP_HIPCHK(hipHostMalloc(&h->h_results, 1 << 17, hipHostMallocDefault));
    h->h_results_cap = 1 << 17;
    if (const char* e = std::getenv("RLAP_PHASE_PROFILE")) { if (e[0] == '1') ENSURE(h->prof, 8 * 80); }
    if (const char* e = std::getenv("RLAP_DEBUG_POISON")) { if (e[0]) h->poison = std::atoi(e) & 0xFF; }
    if (const char* e = std::getenv("RLAP_DEBUG_JITTER")) { if (e[0]) h->jitter = std::max(0, std::min(64, std::atoi(e))); }
    return RLAP_OK;
}

int rlap_create(rlap_handle* out) {
    if (!out) return RLAP_E_BAD_ARG;
    int dev = 0;
    RLAP_HIPCHK(hipGetDevice(&dev));
    rlap_handle h = new rlap_handle_s();
    h->device = dev;
    if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || h->n_cu <= 0) h->n_cu = 256;
    for (auto& e : h->ev) e = nullptr;
    for (auto& e : h->fork_ev) e = nullptr;
    const int rc = create_into(h);
    if (rc != RLAP_OK) { (void)rlap_destroy(h); return rc; }
    *out = h;
    return RLAP_OK;
}

int rlap_destroy(rlap_handle h) {
    if (!h) return RLAP_OK;
    DeviceGuard dg(h->device);
    if (h->h_results) (void)hipHostFree(h->h_results);
    h->own_ws.release(); h->own_rng.release(); h->eqtab.release(); h->prof.release(); h->trace.release(); h->small.release();
    for (auto& e : h->ev) if (e) (void)hipEventDestroy(e);
    for (auto& e : h->fork_ev) if (e) (void)hipEventDestroy(e);
    for (auto& st : h->side) if (st) (void)hipStreamDestroy(st);
    delete h;
    return RLAP_OK;
}

// ---- workspace contract ("caller owns every buffer"; the reference lets torch allocate, py_api_binder.cc:42) ----
static int ws_query(const rlap_handle h, int64_t E, int64_t n_total, int64_t G, int symmetrize, size_t* ws_bytes, int64_t* rng_entries) {
    if (E < 0 || n_total < 0 || G < 1) return RLAP_E_BAD_ARG;
    const int64_t Eeff = symmetrize ? 2 * E : E;
    if (n_total >= (int64_t)1 << 30 || Eeff >= (int64_t)1 << 31 || G >= (int64_t)1 << 30) return RLAP_E_TOO_LARGE;
    rlap_handle_s defaults;   // (growth factors of a fresh handle when none is given)
    const rlap_handle hh = h ? h : &defaults;
    Sizes z;
    // bounds that hold for every split of n_total over G graphs and every num_remove: 2n+1 buckets per graph, S <= n_total
    // (the degree order's squeeze passes are part of the bound wherever a call of these sizes could run them)
    int rc = call_sizes(hh, Eeff, n_total, G, 2 * n_total + G, n_total, true, flow_wanted(hh, OV_RANDOM, G, n_total), n_total, &z, 0,
                        squeeze_passes(OV_DEGREE, (unsigned)G, hh->n_cu, false, false, Eeff));
    if (rc) return rc;
    WS W; Carve dry{nullptr, 0};
    *ws_bytes = carve(dry, z, W);
    *rng_entries = rng_guess(hh, Eeff, G);
    return RLAP_OK;
}

int rlap_workspace_bytes(int64_t E, int64_t n_total, int64_t G, int symmetrize, size_t* ws_bytes, int64_t* rng_entries) {
    if (!ws_bytes || !rng_entries) return RLAP_E_BAD_ARG;
    return ws_query(nullptr, E, n_total, G, symmetrize, ws_bytes, rng_entries);
}

int rlap_workspace_query(rlap_handle h, int64_t E, int64_t n_total, int64_t G, int symmetrize, size_t* ws_bytes, int64_t* rng_entries) {
    if (!h || !ws_bytes || !rng_entries) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return ws_query(h, E, n_total, G, symmetrize, ws_bytes, rng_entries);
}

int rlap_set_workspace(rlap_handle h, void* d_ws, size_t ws_bytes, double* d_rng, int64_t rng_entries) {
    if (!h || (d_ws && (reinterpret_cast<uintptr_t>(d_ws) & 255)) || rng_entries < 0) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    DeviceGuard dg(h->device);
    h->ext_ws = d_ws; h->ext_ws_bytes = d_ws ? ws_bytes : 0;
    if (d_ws) h->own_ws.release();
    if (d_rng != h->ext_rng || rng_entries != h->ext_rng_cap || (!d_rng && h->rng_ptr != h->own_rng.as<double>())) { h->rng_ptr = nullptr; h->rng_len = 0; }   // a table in another buffer is generated anew
    h->ext_rng = d_rng; h->ext_rng_cap = d_rng ? rng_entries : 0;
    if (d_rng) h->own_rng.release();
    return RLAP_OK;
}

int rlap_workspace_needed(rlap_handle h, size_t* ws_bytes, int64_t* rng_entries) {
    if (!h || !ws_bytes || !rng_entries) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    *ws_bytes = h->ws_needed; *rng_entries = h->rng_needed;
    return RLAP_OK;
}

int rlap_set_stream(rlap_handle h, void* hip_stream) {
    if (!h) return RLAP_E_BAD_ARG;
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);
    return RLAP_OK;
}

int rlap_set_rng_mode(rlap_handle h, int mode) {
    if (!h || (mode != 0 && mode != 1)) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->rng_mode = mode;
    return RLAP_OK;
}

int rlap_set_timing(rlap_handle h, int enable) {
    if (!h) return RLAP_E_BAD_ARG;
    h->timing = enable != 0;
    return RLAP_OK;
}

const char* rlap_status_string(int status) {
    switch (status) {
        case RLAP_OK: return "ok";
        case RLAP_E_NOT_SYMMETRIC: return "adjacency matrix is not symmetric";
        case RLAP_E_INDEX_RANGE: return "edge index out of range [0, num_nodes)";
        case RLAP_E_BAD_ARG: return "bad argument";
        case RLAP_E_POOL_OVERFLOW: return "append pool exhausted";
        case RLAP_E_LOG_OVERFLOW: return "priority-queue log exhausted";
        case RLAP_E_RNG_OVERFLOW: return "uniform table exhausted";
        case RLAP_E_OUT_OVERFLOW: return "output buffer too small";
        case RLAP_E_HIP: return "HIP runtime error";
        case RLAP_E_TOO_LARGE: return "problem exceeds int32 slot ids";
        case RLAP_E_WORKSPACE: return "caller-provided workspace too small (see rlap_workspace_needed)";
        case RLAP_E_NOT_GROUPED: return "a column's rows are not contiguous within a segment";
        case RLAP_E_OUT_CAPACITY: return "output capacity too small (rlap_ppr_info.rows_needed says how many rows)";
        default: return "internal error";
    }
}

int rlap_identity(rlap_handle h, const double* d_in, double* d_tmp, double* d_out, int64_t rows, int64_t cols) {
    if (!h || rows < 0 || cols < 0) return RLAP_E_BAD_ARG;
    int64_t total = rows * cols;
    if (total == 0) return RLAP_OK;
    hipLaunchKernelGGL(k_transpose_copy, dim3(nblk(total, 256)), dim3(256), 0, h->stream, d_in, d_tmp, rows, cols, 1);
    hipLaunchKernelGGL(k_transpose_copy, dim3(nblk(total, 256)), dim3(256), 0, h->stream, (const double*)d_tmp, d_out, rows, cols, 0);
    RLAP_HIPCHK(hipGetLastError());
    RLAP_HIPCHK(hipStreamSynchronize(h->stream));
    return RLAP_OK;
}

int rlap_unpack_edge_info(rlap_handle h, const double* d_edge_info, int64_t E, int64_t* d_row, int64_t* d_col, double* d_w) {
    if (!h || E < 0) return RLAP_E_BAD_ARG;
    if (E == 0) return RLAP_OK;
    hipLaunchKernelGGL(k_unpack_edge_info, dim3(nblk(E, 256)), dim3(256), 0, h->stream, d_edge_info, E, d_row, d_col, d_w);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int rlap_pack_rows(rlap_handle h, const double* d_sc, int64_t rows, void* d_packed) {
    if (!h || rows < 0) return RLAP_E_BAD_ARG;
    if (rows == 0) return RLAP_OK;
    DeviceGuard dg(h->device);
    hipLaunchKernelGGL(k_pack_rows, dim3(nblk(rows, 256)), dim3(256), 0, h->stream, d_sc, rows, reinterpret_cast<unsigned long long*>(d_packed));
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int rlap_unpack_rows(rlap_handle h, const void* d_packed, int64_t rows, double* d_sc) {
    if (!h || rows < 0) return RLAP_E_BAD_ARG;
    if (rows == 0) return RLAP_OK;
    DeviceGuard dg(h->device);
    hipLaunchKernelGGL(k_unpack_rows, dim3(nblk(rows, 256)), dim3(256), 0, h->stream, reinterpret_cast<const unsigned long long*>(d_packed), rows, d_sc);
    RLAP_HIPCHK(hipGetLastError());
    return RLAP_OK;
}

int rlap_approx_chol_batched(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E, int64_t G,
                             const int64_t* h_node_ptr, const int64_t* h_num_remove, int o_v, int o_n, const int64_t* d_perm,
                             uint64_t shuffle_seed, double* d_out, int64_t out_cap_rows, int64_t* h_out_row_ptr, rlap_stats* h_stats) {
    return eliminate(h, {.d_row = d_row, .d_col = d_col, .d_w = d_w, .E = E, .G = G, .h_node_ptr = h_node_ptr, .h_num_remove = h_num_remove,
                         .o_v = o_v, .o_n = o_n, .d_perm = d_perm, .seed = shuffle_seed, .d_out = d_out, .out_cap = out_cap_rows,
                         .h_out_ptr = h_out_row_ptr, .st = h_stats});
}

int rlap_approx_chol_views(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E, int64_t G,
                           const int64_t* h_node_ptr, int64_t K, const int64_t* h_num_remove, int o_v, int o_n, const int64_t* d_perm,
                           uint64_t shuffle_seed, double* d_out, int64_t out_cap_rows, int64_t* h_out_ptr, rlap_stats* h_stats) {
    return eliminate(h, {.d_row = d_row, .d_col = d_col, .d_w = d_w, .E = E, .G = G, .h_node_ptr = h_node_ptr, .K = K,
                         .h_num_remove = h_num_remove, .o_v = o_v, .o_n = o_n, .d_perm = d_perm, .seed = shuffle_seed, .d_out = d_out,
                         .out_cap = out_cap_rows, .h_out_ptr = h_out_ptr, .st = h_stats});
}

int rlap_approx_chol_depths(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E, int64_t n,
                            int64_t K, const int64_t* h_num_remove, int o_v, int o_n, const int64_t* d_perm, uint64_t shuffle_seed,
                            double* d_out, int64_t out_cap_rows, int64_t* h_out_ptr, rlap_stats* h_stats) {
    if (K < 1) return RLAP_E_BAD_ARG;   // (D = 0 is a call without depths)
    const int64_t node_ptr[2] = {0, n};
    return eliminate(h, {.d_row = d_row, .d_col = d_col, .d_w = d_w, .E = E, .h_node_ptr = node_ptr, .D = K, .h_num_remove = h_num_remove,
                         .o_v = o_v, .o_n = o_n, .d_perm = d_perm, .seed = shuffle_seed, .d_out = d_out, .out_cap = out_cap_rows,
                         .h_out_ptr = h_out_ptr, .st = h_stats});
}

int rlap_approx_chol_views_depths(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E,
                                  int64_t G, const int64_t* h_node_ptr, int64_t K, int64_t D, const int64_t* h_num_remove,
                                  int o_v, int o_n, const int64_t* d_perm, uint64_t shuffle_seed,
                                  double* d_out, int64_t out_cap_rows, int64_t* h_out_ptr, rlap_stats* h_stats) {
    if (D < 1) return RLAP_E_BAD_ARG;
    return eliminate(h, {.d_row = d_row, .d_col = d_col, .d_w = d_w, .E = E, .G = G, .h_node_ptr = h_node_ptr, .K = K, .D = D,
                         .h_num_remove = h_num_remove, .o_v = o_v, .o_n = o_n, .d_perm = d_perm, .seed = shuffle_seed, .d_out = d_out,
                         .out_cap = out_cap_rows, .h_out_ptr = h_out_ptr, .st = h_stats});
}

int rlap_approx_chol(rlap_handle h, const int64_t* d_row, const int64_t* d_col, const double* d_w, int64_t E, int64_t n, int64_t t,
                     int o_v, int o_n, const int64_t* d_perm, uint64_t shuffle_seed, double* d_out, int64_t out_cap_rows,
                     int64_t* h_out_rows, rlap_stats* h_stats) {
    if (!h_out_rows) return RLAP_E_BAD_ARG;
    const int64_t node_ptr[2] = {0, n};
    int64_t rp[2] = {0, 0};
    const int rc = eliminate(h, {.d_row = d_row, .d_col = d_col, .d_w = d_w, .E = E, .h_node_ptr = node_ptr, .h_num_remove = &t, .o_v = o_v,
                                 .o_n = o_n, .d_perm = d_perm, .seed = shuffle_seed, .d_out = d_out, .out_cap = out_cap_rows,
                                 .h_out_ptr = rp, .st = h_stats});
    *h_out_rows = rp[1];
    return rc;
}

int rlap_approx_chol_from_edges(rlap_handle h, const int64_t* d_src, const int64_t* d_dst, const double* d_w, int64_t E, int64_t n, int64_t t,
                                double remove_frac, int symmetrize, int o_v, int o_n, const int64_t* d_perm, uint64_t shuffle_seed,
                                double* d_out, int64_t out_cap_rows, int64_t* h_out_rows, int64_t* h_num_nodes, rlap_stats* h_stats) {
    if (!h_out_rows) return RLAP_E_BAD_ARG;
    if (n < 0) {
        // num_nodes = edge_index.max() + 1 (augmentor_benchmarks.py:77): one reduction + one 8-byte read-back, after the checks of
        // what it reads (an injected node_id vector needs a known num_nodes); the other checks follow in eliminate()
        if (!h || E < 0 || (E > 0 && (!d_src || !d_dst)) || d_perm) return RLAP_E_BAD_ARG;
        std::lock_guard<std::mutex> lock(h->mu);
        DeviceGuard dg(h->device);
        unsigned long long mx[2] = {0ull, 0ull};   // max id + 1, any id negative
        if (E > 0) {
            unsigned long long* d_mx = h->small.as<unsigned long long>();
            RLAP_HIPCHK(hipMemsetAsync(d_mx, 0, 16, h->stream));
            hipLaunchKernelGGL(k_max_id, dim3((unsigned)std::min<int64_t>((E + 255) / 256, 1024)), dim3(256), 0, h->stream, d_src, d_dst, E, d_mx);
            RLAP_HIPCHK(hipMemcpyAsync(mx, d_mx, 16, hipMemcpyDeviceToHost, h->stream));
            RLAP_HIPCHK(hipStreamSynchronize(h->stream));
        }
        if (mx[1]) return RLAP_E_INDEX_RANGE;   // a negative id is out of range for every num_nodes (an explicit n reports the same)
        n = (int64_t)mx[0];
    }
    if (t < 0) t = (int64_t)(remove_frac * (double)n);   // int(frac * num_nodes), augmentor_benchmarks.py:78
    if (h_num_nodes) *h_num_nodes = n;
    const int64_t node_ptr[2] = {0, n};
    int64_t rp[2] = {0, 0};
    const int rc = eliminate(h, {.d_row = d_src, .d_col = d_dst, .d_w = d_w, .E = E, .h_node_ptr = node_ptr, .h_num_remove = &t, .o_v = o_v,
                                 .o_n = o_n, .d_perm = d_perm, .seed = shuffle_seed, .d_out = d_out, .out_cap = out_cap_rows,
                                 .h_out_ptr = rp, .symmetrize = symmetrize ? 1 : 0, .st = h_stats});
    *h_out_rows = rp[1];
    return rc;
}

}  // extern "C"

namespace {

// The checks the five snapshot exports share (their own RLAP_E_BAD_ARG checks come before this, their own size limits behind it):
// the handle and the tables are there, at least min_S segments, G graphs divide them (G = 1 without node_ptr), and m and S fit
// the int32 row and block numbers.
int snapshot_check(rlap_handle h, SnapshotSeg* g, int64_t min_S) {
    if (!h || !g->ptr || g->S < min_S || g->m < 0 || g->N < 0 || (g->m > 0 && !g->sc)) return RLAP_E_BAD_ARG;
    if (g->node_ptr ? (g->G < 1 || g->S % g->G != 0) : false) return RLAP_E_BAD_ARG;
    if (!g->node_ptr) g->G = 1;
    if (g->m >= INT32_MAX || g->S >= (int64_t)1 << 30) return RLAP_E_TOO_LARGE;
    return RLAP_OK;
}

// One snapshot call on the handle: its lock, its device, an arena of bytes() bytes, then run(base, have, need) -> status.
template <class Bytes, class Run>
int snapshot_call(rlap_handle h, Bytes bytes, Run run) {
    std::lock_guard<std::mutex> lock(h->mu);
    DeviceGuard dg(h->device);
    const size_t need = bytes();
    void* base = nullptr;
    size_t have = 0;
    if (const int rc = arena(h, need, &base, &have)) return rc;
    return run(base, have, need);
}

// One call of the readout, the fused losses or the probe on that path.  A poisoned handle (debug) first fills the arena and the
// result buffers `outs` -- (pointer, bytes); a null pointer or zero bytes is skipped -- so that no result can depend on what they
// held.  *arena_bytes (may be null) gets the arena's size; then run(base, have) -> status.
using PoisonList = std::initializer_list<std::pair<void*, size_t>>;
template <class Bytes, class Run>
int poisoned_call(rlap_handle h, Bytes bytes, PoisonList outs, int64_t* arena_bytes, Run run) {
    return snapshot_call(h, bytes, [&](void* base, size_t have, size_t need) -> int {
        if (h->poison >= 0) {
            if (need) RLAP_HIPCHK(hipMemsetAsync(base, h->poison, need, h->stream));
            for (const auto& o : outs)
                if (o.first && o.second) RLAP_HIPCHK(hipMemsetAsync(o.first, h->poison, o.second, h->stream));
        }
        if (arena_bytes) *arena_bytes = (int64_t)need;
        return run(base, have);
    });
}

}  // namespace

extern "C" {

int rlap_snapshot_stats(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                        int64_t G, int64_t num_nodes, int weighted, double tol, int32_t max_iter, int64_t* d_nodes,
                        double* d_lambda_max, int32_t* d_iters, int32_t* d_converged, rlap_snapshot_info* h_info) {
    if (!d_nodes || !d_lambda_max || !d_iters || !d_converged) return RLAP_E_BAD_ARG;
    if (!(tol > 0.0) || !std::isfinite(tol) || max_iter < 1 || max_iter > STATS_MAX_ITER) return RLAP_E_BAD_ARG;
    SnapshotSeg g{d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes};
    if (const int rc = snapshot_check(h, &g, 1)) return rc;   // (no limit on num_nodes: the id slots are counted in 64 bits)
    const SnapshotStatsArgs a{g, weighted, tol, max_iter, d_nodes, d_lambda_max, d_iters, d_converged};
    return snapshot_call(h, [&] { return snapshot_stats_bytes(g.m, g.S, g.G, g.N, max_iter); }, [&](void* base, size_t have, size_t) {
        SnapshotStatsReport rep;
        const int rc = snapshot_stats_run(h->stream, base, have, a, &rep);
        if (h_info) {
            h_info->small_segments = rep.small_segments; h_info->large_segments = rep.large_segments;
            h_info->lanczos_steps = rep.lanczos_steps; h_info->large_steps = rep.large_steps; h_info->large_launches = rep.large_launches;
            h_info->host_syncs = rep.host_syncs; h_info->not_converged = rep.not_converged;
        }
        return rc;
    });
}

int rlap_snapshot_ppr(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                      int64_t G, int64_t num_nodes, double alpha, double eps, double tol, int flags, double* d_out,
                      int64_t out_cap_rows, int64_t* d_out_ptr, rlap_ppr_info* h_info) {
    if (h_info) *h_info = rlap_ppr_info{};
    if (!d_out_ptr || out_cap_rows < 0 || (out_cap_rows > 0 && !d_out)) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_PPR_WEIGHTED | RLAP_PPR_SELF_LOOP | RLAP_PPR_NORMALIZE | RLAP_PPR_ZERO_ROWS)) return RLAP_E_BAD_ARG;
    if (!(eps > 0.0) || !std::isfinite(eps)) return RLAP_E_BAD_ARG;
    const int K = cheb::steps(alpha, tol, cheb::MAX_STEPS);
    if (K < 0) return RLAP_E_BAD_ARG;
    SnapshotSeg g{d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes};
    if (const int rc = snapshot_check(h, &g, 1)) return rc;
    if (num_nodes >= INT32_MAX) return RLAP_E_TOO_LARGE;
    const SnapshotPprArgs a{g, alpha, eps, K, flags, d_out, out_cap_rows, d_out_ptr};
    return snapshot_call(h, [&] { return snapshot_ppr_bytes(g.m, g.S, g.G, g.N, out_cap_rows, K); }, [&](void* base, size_t have, size_t need) {
        SnapshotPprReport rep;
        const int rc = snapshot_ppr_run(h->stream, base, have, a, &rep);
        if (h_info) {
            h_info->steps = K; h_info->small_tiles = rep.small_tiles; h_info->large_tiles = rep.large_tiles; h_info->groups = rep.groups;
            h_info->launches = rep.launches; h_info->rows_needed = rep.kept; h_info->arena_bytes = (int64_t)need;
            h_info->host_syncs = rep.host_syncs;
        }
        return rc;
    });
}

int rlap_snapshot_markov(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                         int64_t G, int64_t num_nodes, double alpha, int32_t order, double eps, int flags, double* d_out,
                         int64_t out_cap_rows, int64_t* d_out_ptr, rlap_markov_info* h_info) {
    if (h_info) *h_info = rlap_markov_info{};
    if (!d_out_ptr || out_cap_rows < 0 || (out_cap_rows > 0 && !d_out)) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_MARKOV_WEIGHTED | RLAP_MARKOV_SELF_LOOP | RLAP_MARKOV_NORMALIZE | RLAP_MARKOV_ZERO_ROWS)) return RLAP_E_BAD_ARG;
    if (!markov::valid(alpha, order, eps)) return RLAP_E_BAD_ARG;
    SnapshotSeg g{d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes};
    if (const int rc = snapshot_check(h, &g, 1)) return rc;
    if (num_nodes >= INT32_MAX) return RLAP_E_TOO_LARGE;
    const SnapshotMarkovArgs a{g, alpha, eps, order, flags, d_out, out_cap_rows, d_out_ptr};
    return snapshot_call(h, [&] { return snapshot_markov_bytes(g.m, g.S, g.G, g.N, out_cap_rows); }, [&](void* base, size_t have, size_t need) {
        SnapshotMarkovReport rep;
        const int rc = snapshot_markov_run(h->stream, base, have, a, &rep);
        if (h_info) {
            h_info->order = order; h_info->small_tiles = rep.small_tiles;
            h_info->large_tiles = rep.large_tiles; h_info->groups = rep.groups; h_info->launches = rep.launches;
            h_info->rows_needed = rep.kept; h_info->arena_bytes = (int64_t)need; h_info->host_syncs = rep.host_syncs;
        }
        return rc;
    });
}

int rlap_snapshot_subgraph(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                           int64_t G, int64_t num_nodes, const int64_t* d_nodes, const int64_t* d_nodes_ptr, int64_t nodes_len,
                           int flags, double* d_out, int64_t* d_out_ptr, int64_t* d_ids, int64_t ids_cap, int64_t* d_ids_ptr,
                           rlap_subgraph_info* h_info) {
    if (h_info) *h_info = rlap_subgraph_info{};
    if ((m > 0 && (!d_out || S < 1)) || !d_out_ptr || !d_ids_ptr) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_SUB_RELABEL | RLAP_SUB_NO_SELF_LOOPS)) return RLAP_E_BAD_ARG;
    if (d_nodes ? nodes_len < 0 : (d_nodes_ptr != nullptr)) return RLAP_E_BAD_ARG;   // (nodes_ptr only together with nodes)
    if (!d_nodes) nodes_len = 0;
    SnapshotSeg g{d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes};
    if (const int rc = snapshot_check(h, &g, 0)) return rc;   // (S == 0: no segment at all, and then no rows)
    if (num_nodes >= INT32_MAX || nodes_len >= INT32_MAX || (g.S / g.G) * num_nodes >= (int64_t)1 << 40) return RLAP_E_TOO_LARGE;
    const int64_t ids_need = snapshot_subgraph_ids_cap(g.m, g.S, g.G, g.N, d_nodes != nullptr, d_nodes_ptr != nullptr, nodes_len);
    if (ids_cap < ids_need || (ids_need > 0 && !d_ids)) return RLAP_E_BAD_ARG;
    const SnapshotSubArgs a{g, d_nodes, d_nodes_ptr, nodes_len, flags, d_out, d_out_ptr, d_ids, ids_cap, d_ids_ptr};
    return snapshot_call(h, [&] { return snapshot_subgraph_bytes(g.m, g.S, g.G, g.N); }, [&](void* base, size_t have, size_t need) {
        SnapshotSubReport rep;
        const int rc = snapshot_subgraph_run(h->stream, base, have, a, &rep);
        if (h_info) {
            h_info->rows_kept = rep.kept; h_info->ids_written = rep.ids; h_info->arena_bytes = (int64_t)need; h_info->host_syncs = rep.host_syncs;
        }
        return rc;
    });
}

int rlap_snapshot_gcn_norm(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                           int64_t G, int64_t num_nodes, int flags, double fill_value, int64_t* d_src, int64_t* d_dst, void* d_val,
                           int64_t cap, int64_t* d_eptr, rlap_gcn_info* h_info) {
    if (h_info) *h_info = rlap_gcn_info{};
    if (!d_eptr || cap < 0) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_GCN_WEIGHTED | RLAP_GCN_SELF_LOOPS | RLAP_GCN_NORMALIZE | RLAP_GCN_F32)) return RLAP_E_BAD_ARG;
    if ((flags & RLAP_GCN_SELF_LOOPS) && !(fill_value > 0.0 && std::isfinite(fill_value))) return RLAP_E_BAD_ARG;
    SnapshotSeg g{d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes};
    if (const int rc = snapshot_check(h, &g, 1)) return rc;
    if (num_nodes >= INT32_MAX || (g.S / g.G) * num_nodes >= (int64_t)1 << 40) return RLAP_E_TOO_LARGE;
    const int64_t cap_need = snapshot_gcn_cap(g.m, g.S, g.G, g.N, flags);
    if (cap < cap_need || (cap_need > 0 && (!d_src || !d_dst || !d_val))) return RLAP_E_BAD_ARG;
    const SnapshotGcnArgs a{g, flags, fill_value, d_src, d_dst, d_val, d_eptr};
    return snapshot_call(h, [&] { return snapshot_gcn_bytes(g.m, g.S, g.G, g.N); }, [&](void* base, size_t have, size_t need) {
        SnapshotGcnReport rep;
        const int rc = snapshot_gcn_run(h->stream, base, have, a, &rep);
        if (h_info) {
            h_info->entries = rep.entries; h_info->loops_removed = rep.loops_removed; h_info->arena_bytes = (int64_t)need;
            h_info->host_syncs = rep.host_syncs;
        }
        return rc;
    });
}

int rlap_snapshot_propagate(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                            int64_t G, int64_t num_nodes, int flags, double fill_value, const void* d_x, int64_t F, void* d_y,
                            rlap_spmm_info* h_info) {
    if (h_info) *h_info = rlap_spmm_info{};
    if (F < 1) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_GCN_WEIGHTED | RLAP_GCN_SELF_LOOPS | RLAP_GCN_NORMALIZE | RLAP_SPMM_TRANSPOSE | RLAP_SPMM_X_F32 | RLAP_SPMM_X_PER_LAYER))
        return RLAP_E_BAD_ARG;
    if ((flags & RLAP_GCN_SELF_LOOPS) && !(fill_value > 0.0 && std::isfinite(fill_value))) return RLAP_E_BAD_ARG;
    SnapshotSeg g{d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes};
    if (const int rc = snapshot_check(h, &g, 1)) return rc;
    if (num_nodes >= INT32_MAX || F > SPMM_MAX_F) return RLAP_E_TOO_LARGE;
    if ((g.S / g.G) * num_nodes >= SPMM_MAX_ELEMS || (g.S / g.G) * num_nodes * F >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    const int64_t elems = (g.S / g.G) * num_nodes * F;
    if (elems > 0 && (!d_x || !d_y)) return RLAP_E_BAD_ARG;
    return snapshot_call(h, [&] { return snapshot_spmm_bytes(g.m, g.S, g.G, g.N, F, flags, h->dbg_scr); }, [&](void* base, size_t have, size_t need) -> int {
        if (h->poison >= 0) {   // debug: the result must not depend on what the arena or the result buffer held
            RLAP_HIPCHK(hipMemsetAsync(base, h->poison, need, h->stream));
            if (elems > 0) RLAP_HIPCHK(hipMemsetAsync(d_y, h->poison, (size_t)elems * ((flags & RLAP_SPMM_X_F32) ? 4 : 8), h->stream));
        }
        const SnapshotSpmmArgs a{g, flags, fill_value, d_x, F, d_y, h->dbg_scr};
        SnapshotSpmmReport rep;
        const int rc = snapshot_spmm_run(h->stream, base, have, a, &rep);
        if (h_info) {
            h_info->entries = rep.entries; h_info->blocks = rep.blocks; h_info->chunked_lists = rep.chunked_lists;
            h_info->arena_bytes = (int64_t)need; h_info->host_syncs = rep.host_syncs;
        }
        return rc;
    });
}

int rlap_snapshot_plan_bytes(int64_t m, int64_t S, int64_t G, int64_t num_nodes, int flags, size_t* bytes) {
    if (!bytes || m < 0 || S < 1 || G < 1 || num_nodes < 0 || S % G != 0) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_GCN_WEIGHTED | RLAP_GCN_SELF_LOOPS | RLAP_GCN_NORMALIZE | RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED)) return RLAP_E_BAD_ARG;
    if (m >= INT32_MAX || S >= (int64_t)1 << 30 || num_nodes >= INT32_MAX || (S / G) * num_nodes >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    if (!(flags & (RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED))) flags |= RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED;
    *bytes = snapshot_plan_buffer_bytes(m, S, G, num_nodes, flags);
    return RLAP_OK;
}

int rlap_snapshot_plan_build(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                             int64_t G, int64_t num_nodes, int flags, double fill_value, void* d_plan, size_t plan_bytes,
                             rlap_plan_desc* h_desc, rlap_plan_info* h_info) {
    if (h_info) *h_info = rlap_plan_info{};
    if (!h_desc) return RLAP_E_BAD_ARG;
    *h_desc = rlap_plan_desc{};
    if (!d_plan || (reinterpret_cast<uintptr_t>(d_plan) & 15)) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_GCN_WEIGHTED | RLAP_GCN_SELF_LOOPS | RLAP_GCN_NORMALIZE | RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED)) return RLAP_E_BAD_ARG;
    if ((flags & RLAP_GCN_SELF_LOOPS) && !(fill_value > 0.0 && std::isfinite(fill_value))) return RLAP_E_BAD_ARG;
    if (!(flags & (RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED))) flags |= RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED;
    SnapshotSeg g{d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes};
    if (const int rc = snapshot_check(h, &g, 1)) return rc;
    if (num_nodes >= INT32_MAX || (g.S / g.G) * num_nodes >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    if (plan_bytes < snapshot_plan_buffer_bytes(g.m, g.S, g.G, g.N, flags)) return RLAP_E_BAD_ARG;
    return snapshot_call(h, [&] { return snapshot_plan_build_bytes(g.m, g.S, g.G, g.N, flags); }, [&](void* base, size_t have, size_t need) -> int {
        if (h->poison >= 0) {   // debug: the plan must not depend on what the arena or the caller's buffer held
            RLAP_HIPCHK(hipMemsetAsync(base, h->poison, need, h->stream));
            RLAP_HIPCHK(hipMemsetAsync(d_plan, h->poison, plan_bytes, h->stream));
        }
        const SnapshotPlanArgs a{g, flags, fill_value, d_plan, plan_bytes};
        SnapshotPlanReport rep;
        const int rc = snapshot_plan_build_run(h->stream, base, have, a, h_desc, &rep);
        if (rc != RLAP_OK) *h_desc = rlap_plan_desc{};
        if (h_info) {
            h_info->entries = rep.entries; h_info->blocks = rep.blocks; h_info->chunked_lists_forward = rep.chunked[0];
            h_info->chunked_lists_transposed = rep.chunked[1]; h_info->loops_removed = rep.loops_removed;
            h_info->arena_bytes = (int64_t)need; h_info->host_syncs = rep.host_syncs;
        }
        return rc;
    });
}

int rlap_edge_plan_build(rlap_handle h, const double* d_sc, int64_t m, const int64_t* d_ptr, int64_t S, const int64_t* d_node_ptr,
                         int64_t G, int64_t num_nodes, int flags, double fill_value, void* d_plan, size_t plan_bytes,
                         rlap_plan_desc* h_desc, rlap_plan_info* h_info) {
    if (h_info) *h_info = rlap_plan_info{};
    if (!h_desc) return RLAP_E_BAD_ARG;
    *h_desc = rlap_plan_desc{};
    if (!d_plan || (reinterpret_cast<uintptr_t>(d_plan) & 15)) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_GCN_WEIGHTED | RLAP_GCN_SELF_LOOPS | RLAP_GCN_NORMALIZE | RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED)) return RLAP_E_BAD_ARG;
    if ((flags & RLAP_GCN_SELF_LOOPS) && !(fill_value > 0.0 && std::isfinite(fill_value))) return RLAP_E_BAD_ARG;
    if (!(flags & (RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED))) flags |= RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED;
    SnapshotSeg g{d_sc, m, d_ptr, S, d_node_ptr, G, num_nodes};
    if (const int rc = snapshot_check(h, &g, 1)) return rc;
    if (num_nodes >= INT32_MAX || (g.S / g.G) * num_nodes >= edgeplan::MAX_SLOTS) return RLAP_E_TOO_LARGE;   // (rlap_edgeplan.h: uint32 slot keys)
    if (plan_bytes < snapshot_plan_buffer_bytes(g.m, g.S, g.G, g.N, flags)) return RLAP_E_BAD_ARG;
    return snapshot_call(h, [&] { return edge_plan_build_bytes(g.m, g.S, g.G, g.N, flags); }, [&](void* base, size_t have, size_t need) -> int {
        if (h->poison >= 0) {   // debug: the plan must not depend on what the arena or the caller's buffer held
            RLAP_HIPCHK(hipMemsetAsync(base, h->poison, need, h->stream));
            RLAP_HIPCHK(hipMemsetAsync(d_plan, h->poison, plan_bytes, h->stream));
        }
        const SnapshotPlanArgs a{g, flags, fill_value, d_plan, plan_bytes};
        SnapshotPlanReport rep;
        const int rc = edge_plan_build_run(h->stream, base, have, a, h_desc, &rep);
        if (rc != RLAP_OK) *h_desc = rlap_plan_desc{};
        if (h_info) {
            h_info->entries = rep.entries; h_info->blocks = rep.blocks; h_info->chunked_lists_forward = rep.chunked[0];
            h_info->chunked_lists_transposed = rep.chunked[1]; h_info->loops_removed = rep.loops_removed;
            h_info->arena_bytes = (int64_t)need; h_info->host_syncs = rep.host_syncs;
        }
        return rc;
    });
}

int rlap_node_sample(rlap_handle h, const int64_t* d_src, const int64_t* d_dst, const double* d_w, int64_t E, int64_t num_nodes, int scheme,
                     const double* h_p, const int64_t* h_num_seeds, int64_t K, int64_t walk_length, uint64_t seed, double* d_rows,
                     int64_t out_cap_rows, int64_t* d_ptr, uint8_t* d_node_mask, int64_t* d_walks, rlap_node_sample_info* h_info) {
    if (h_info) *h_info = rlap_node_sample_info{};
    if (!h || E < 0 || num_nodes < 0 || (E > 0 && (!d_src || !d_dst)) || K < 1 || !d_ptr) return RLAP_E_BAD_ARG;
    if (out_cap_rows < 0 || (out_cap_rows > 0 && !d_rows)) return RLAP_E_BAD_ARG;
    if (scheme < 0 || scheme >= nodesample::SCHEMES) return RLAP_E_BAD_ARG;
    const bool walk = scheme == RLAP_SAMPLE_WALK;
    if (walk ? !h_num_seeds : !h_p) return RLAP_E_BAD_ARG;
    if (!walk && d_walks) return RLAP_E_BAD_ARG;
    if (E >= INT32_MAX || num_nodes >= (int64_t)1 << 31 || K > nodesample::MAX_VIEWS) return RLAP_E_TOO_LARGE;
    NodeSampleArgs a{};
    int64_t walkers = 0;
    for (int64_t k = 0; k < K; ++k) {
        if (walk) {
            if (h_num_seeds[k] < 0) return RLAP_E_BAD_ARG;
            if (h_num_seeds[k] >= (int64_t)1 << 31) return RLAP_E_TOO_LARGE;
            a.seeds[k] = h_num_seeds[k];
            walkers += h_num_seeds[k];
        } else {
            if (!(h_p[k] >= 0.0 && h_p[k] <= 1.0)) return RLAP_E_BAD_ARG;
            a.p[k] = h_p[k];
        }
    }
    if (walk && (walk_length < 0 || walk_length > nodesample::MAX_WALK_LENGTH || (walkers > 0 && num_nodes == 0))) return RLAP_E_BAD_ARG;
    a.src = d_src; a.dst = d_dst; a.w = d_w; a.E = E; a.N = num_nodes; a.scheme = scheme; a.K = (int)K;
    a.walk_length = walk ? walk_length : 0; a.seed = seed; a.rows = d_rows; a.cap = out_cap_rows; a.ptr = d_ptr;
    a.node_mask = d_node_mask; a.walks = d_walks;
    // (debug poison: no result may depend on what the arena or any of the four result buffers held)
    int64_t arena_bytes = 0;
    NodeSampleReport rep{};
    const int rc = poisoned_call(h, [&] { return node_sample_bytes(E, num_nodes, (int)K, scheme, d_node_mask != nullptr); },
                                 {{d_rows, sizeof(double) * 3 * (size_t)out_cap_rows}, {d_ptr, sizeof(int64_t) * (size_t)(K + 1)},
                                  {d_node_mask, (size_t)K * (size_t)num_nodes}, {d_walks, sizeof(int64_t) * (size_t)walkers * (size_t)(walk_length + 1)}},
                                 &arena_bytes, [&](void* base, size_t have) { return node_sample_run(h->stream, base, have, a, &rep); });
    if (h_info) {
        h_info->rows_needed = rep.rows_needed; h_info->launches = rep.launches; h_info->arena_bytes = arena_bytes;
        h_info->host_syncs = rep.host_syncs;
    }
    return rc;
}

int rlap_edge_add(rlap_handle h, const int64_t* d_src, const int64_t* d_dst, const double* d_w, int64_t E, int64_t num_nodes,
                  const int64_t* h_num_add, int64_t K, uint64_t seed, int flags, double* d_rows, int64_t out_cap_rows, int64_t* d_ptr,
                  int64_t* d_added, int64_t* d_aptr, rlap_edge_add_info* h_info) {
    if (h_info) *h_info = rlap_edge_add_info{};
    if (!h || E < 0 || num_nodes < 0 || (E > 0 && (!d_src || !d_dst)) || !h_num_add || K < 1 || !d_ptr) return RLAP_E_BAD_ARG;
    if (out_cap_rows < 0 || (out_cap_rows > 0 && !d_rows) || (flags & ~RLAP_ADD_COALESCE) || (d_added && !d_aptr)) return RLAP_E_BAD_ARG;
    if (E >= INT32_MAX || num_nodes >= (int64_t)1 << 31 || K > edgeadd::MAX_VIEWS) return RLAP_E_TOO_LARGE;
    EdgeAddArgs a{};
    int64_t added = 0;
    for (int64_t k = 0; k < K; ++k) {
        if (h_num_add[k] < 0) return RLAP_E_BAD_ARG;
        if (h_num_add[k] >= INT32_MAX - E) return RLAP_E_TOO_LARGE;
        a.num_add[k] = h_num_add[k];
        added += h_num_add[k];
    }
    if (added > 0 && (num_nodes < 2 || (d_aptr && !d_added))) return RLAP_E_BAD_ARG;   // (without an added row d_added may be null)
    a.src = d_src; a.dst = d_dst; a.w = d_w; a.E = E; a.N = num_nodes; a.K = (int)K; a.coalesce = (flags & RLAP_ADD_COALESCE) ? 1 : 0;
    a.seed = seed; a.rows = d_rows; a.cap = out_cap_rows; a.ptr = d_ptr; a.added = d_added; a.aptr = d_aptr;
    // (debug poison: no result may depend on what the arena or any of the four result buffers held)
    int64_t arena_bytes = 0;
    EdgeAddReport rep{};
    const int rc = poisoned_call(h, [&] { return edge_add_bytes(E, num_nodes, (int)K, a.num_add, a.coalesce != 0); },
                                 {{d_rows, sizeof(double) * 3 * (size_t)out_cap_rows}, {d_ptr, sizeof(int64_t) * (size_t)(K + 1)},
                                  {d_added, sizeof(int64_t) * 2 * (size_t)added}, {d_aptr, sizeof(int64_t) * (size_t)(K + 1)}},
                                 &arena_bytes, [&](void* base, size_t have) { return edge_add_run(h->stream, base, have, a, &rep); });
    if (h_info) {
        h_info->rows_needed = rep.rows_needed; h_info->added = rep.added; h_info->input_distinct = rep.input_distinct;
        h_info->launches = rep.launches; h_info->arena_bytes = arena_bytes; h_info->input_sorted = rep.input_sorted;
        h_info->sorts = rep.sorts; h_info->host_syncs = rep.host_syncs;
    }
    return rc;
}

int rlap_edge_drop(rlap_handle h, const int64_t* d_src, const int64_t* d_dst, const double* d_w, int64_t E, int64_t num_nodes, int scheme,
                   int flags, const double* h_p, int64_t K, double threshold, uint64_t seed, double pr_damp, int64_t pr_iters,
                   double evc_tol, int64_t evc_max_iter, double* d_rows, int64_t out_cap_rows, int64_t* d_ptr, uint8_t* d_mask,
                   double* d_centrality, double* d_node_weight, rlap_edge_drop_info* h_info) {
    if (h_info) *h_info = rlap_edge_drop_info{};
    if (!h || E < 0 || num_nodes < 0 || (E > 0 && (!d_src || !d_dst)) || !h_p || K < 1 || !d_ptr) return RLAP_E_BAD_ARG;
    if (out_cap_rows < 0 || (out_cap_rows > 0 && !d_rows)) return RLAP_E_BAD_ARG;
    if (scheme < 0 || scheme >= edgedrop::SCHEMES || (flags & ~RLAP_DROP_SOURCE)) return RLAP_E_BAD_ARG;
    if (E >= INT32_MAX || num_nodes >= (int64_t)1 << 31 || K > edgedrop::MAX_VIEWS) return RLAP_E_TOO_LARGE;
    if (!(threshold >= 0.0 && threshold <= 1.0)) return RLAP_E_BAD_ARG;
    for (int64_t k = 0; k < K; ++k)
        if (!(h_p[k] >= 0.0 && h_p[k] <= 1.0)) return RLAP_E_BAD_ARG;
    if (scheme == RLAP_DROP_PAGERANK && (!(pr_damp >= 0.0 && pr_damp <= 1.0) || pr_iters < 0)) return RLAP_E_BAD_ARG;
    if (scheme == RLAP_DROP_EIGENVECTOR && (!(evc_tol >= 0.0) || !std::isfinite(evc_tol) || evc_max_iter < 1)) return RLAP_E_BAD_ARG;
    if ((scheme == RLAP_DROP_PAGERANK && pr_iters > edgedrop::MAX_PR_ITERS) || (scheme == RLAP_DROP_EIGENVECTOR && evc_max_iter > edgedrop::MAX_EVC_ITERS))
        return RLAP_E_TOO_LARGE;
    EdgeDropArgs a{};
    a.src = d_src; a.dst = d_dst; a.w = d_w; a.E = E; a.N = num_nodes; a.scheme = scheme; a.source = (flags & RLAP_DROP_SOURCE) ? 1 : 0;
    for (int64_t k = 0; k < K; ++k) a.p[k] = h_p[k];
    a.K = (int)K; a.threshold = threshold; a.seed = seed; a.damp = pr_damp; a.pr_iters = pr_iters; a.evc_tol = evc_tol;
    a.evc_max_iter = evc_max_iter; a.rows = d_rows; a.cap = out_cap_rows; a.ptr = d_ptr; a.mask = d_mask; a.centrality = d_centrality;
    a.node_weight = d_node_weight;
    // (debug poison: no result may depend on what the arena or any of the five result buffers held)
    const size_t nodes = (size_t)num_nodes, KE = (size_t)K * (size_t)E;
    int64_t arena_bytes = 0;
    EdgeDropReport rep{};
    const int rc = poisoned_call(h, [&] { return edge_drop_bytes(E, num_nodes, (int)K, scheme); },
                                 {{d_rows, sizeof(double) * 3 * (size_t)out_cap_rows}, {d_ptr, sizeof(int64_t) * (size_t)(K + 1)}, {d_mask, KE},
                                  {d_centrality, sizeof(double) * nodes}, {d_node_weight, sizeof(double) * nodes}},
                                 &arena_bytes, [&](void* base, size_t have) { return edge_drop_run(h->stream, base, have, a, &rep); });
    if (h_info) {
        h_info->rows_needed = rep.rows_needed; h_info->launches = rep.launches; h_info->arena_bytes = arena_bytes;
        h_info->iters = rep.iters; h_info->converged = rep.converged; h_info->host_syncs = rep.host_syncs;
    }
    return rc;
}

int rlap_snapshot_plan_propagate(rlap_handle h, const void* d_plan, const rlap_plan_desc* h_desc, int flags, const void* d_x, int64_t F,
                                 void* d_y, rlap_spmm_info* h_info) {
    if (h_info) *h_info = rlap_spmm_info{};
    if (!h || !d_plan || !h_desc || F < 1) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_SPMM_TRANSPOSE | RLAP_SPMM_X_F32 | RLAP_SPMM_X_PER_LAYER)) return RLAP_E_BAD_ARG;
    const rlap_plan_desc d = *h_desc;
    // a descriptor that a successful build wrote: every part it names lies inside the bytes it reports
    if (d.magic != plan::MAGIC || d.m < 0 || d.m >= INT32_MAX || d.num_nodes < 0 || d.num_nodes >= INT32_MAX || d.graphs < 1 ||
        d.segments < 1 || d.segments >= (int64_t)1 << 30 || d.segments % d.graphs != 0 || (reinterpret_cast<uintptr_t>(d_plan) & 15))
        return RLAP_E_BAD_ARG;
    const int64_t slots = (d.segments / d.graphs) * d.num_nodes;
    if (slots >= SPMM_MAX_ELEMS) return RLAP_E_BAD_ARG;
    const bool t = (flags & RLAP_SPMM_TRANSPOSE) != 0;
    if (!(d.flags & (t ? RLAP_PLAN_TRANSPOSED : RLAP_PLAN_FORWARD))) return RLAP_E_BAD_ARG;
    {
        const int64_t ent = t ? d.entries_transposed : d.entries_forward, ch = t ? d.chunks_transposed : d.chunks_forward;
        const int64_t off = t ? d.off_transposed : d.off_forward, dir = t ? d.dir_transposed : d.dir_forward, rec = t ? d.rec_transposed : d.rec_forward;
        if (ent < 0 || ent > d.m || ch < 0 || ch > plan::dir_cap(d.m) || off < 0 || dir < 0 || rec < 0 || ((off | dir | rec) & 15) ||
            off + 8 * (slots + 1) > d.plan_bytes || dir + 16 * ch > d.plan_bytes || rec + 16 * ent > d.plan_bytes)
            return RLAP_E_BAD_ARG;
        if ((d.flags & RLAP_GCN_SELF_LOOPS) && (d.loop_offset < 0 || (d.loop_offset & 7) || d.loop_offset + 8 * slots > d.plan_bytes)) return RLAP_E_BAD_ARG;
    }
    if (F > SPMM_MAX_F || slots * F >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    const int64_t elems = slots * F;
    if (elems > 0 && (!d_x || !d_y)) return RLAP_E_BAD_ARG;
    return snapshot_call(h, [&] { return snapshot_plan_use_bytes(d, F, flags, h->dbg_scr); }, [&](void* base, size_t have, size_t need) -> int {
        if (h->poison >= 0) {   // debug: the result must not depend on what the arena or the result buffer held
            RLAP_HIPCHK(hipMemsetAsync(base, h->poison, need, h->stream));
            if (elems > 0) RLAP_HIPCHK(hipMemsetAsync(d_y, h->poison, (size_t)elems * ((flags & RLAP_SPMM_X_F32) ? 4 : 8), h->stream));
        }
        const PlanUseArgs a{d_plan, &d, flags, d_x, F, d_y, h->dbg_scr};
        const int rc = snapshot_plan_use_run(h->stream, base, have, a);
        if (h_info) {
            h_info->entries = (t ? d.entries_transposed : d.entries_forward) + ((d.flags & RLAP_GCN_SELF_LOOPS) ? slots : 0);
            h_info->chunked_lists = 0; h_info->blocks = 0;
            h_info->arena_bytes = (int64_t)need; h_info->host_syncs = 0;
        }
        return rc;
    });
}

int rlap_feature_count(rlap_handle h, const void* d_x, int64_t N, int64_t Fin, int flags, int64_t* h_nnz) {
    if (!h || !d_x || !h_nnz || N < 1 || Fin < 1 || (flags & ~RLAP_FEAT_X_F32)) return RLAP_E_BAD_ARG;
    *h_nnz = 0;
    if (N >= featlin::MAX_DIM || Fin >= featlin::MAX_DIM) return RLAP_E_TOO_LARGE;
    return snapshot_call(h, [&] { return feature_count_bytes(N, Fin); }, [&](void* base, size_t have, size_t) -> int {
        return feature_count_run(h->stream, base, have, d_x, N, Fin, flags, h_nnz);
    });
}

int rlap_feature_plan_bytes(int64_t N, int64_t Fin, int64_t nnz, int flags, size_t* bytes) {
    if (!bytes || N < 1 || Fin < 1 || nnz < 0) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_FEAT_X_F32 | RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED)) return RLAP_E_BAD_ARG;
    if (N >= featlin::MAX_DIM || Fin >= featlin::MAX_DIM || nnz >= featlin::MAX_NNZ) return RLAP_E_TOO_LARGE;
    if (!(flags & (RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED))) flags |= RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED;
    *bytes = (size_t)featlin::layout(N, Fin, nnz, (flags & RLAP_PLAN_FORWARD) != 0, (flags & RLAP_PLAN_TRANSPOSED) != 0).bytes;
    return RLAP_OK;
}

int rlap_feature_plan_build(rlap_handle h, const void* d_x, int64_t N, int64_t Fin, int64_t nnz, int flags, void* d_plan, size_t plan_bytes,
                            rlap_feature_desc* h_desc, rlap_feature_info* h_info) {
    if (h_info) *h_info = rlap_feature_info{};
    if (!h_desc) return RLAP_E_BAD_ARG;
    *h_desc = rlap_feature_desc{};
    if (!h || !d_x || !d_plan || (reinterpret_cast<uintptr_t>(d_plan) & 15)) return RLAP_E_BAD_ARG;
    size_t bound = 0;
    if (const int rc = rlap_feature_plan_bytes(N, Fin, nnz, flags, &bound)) return rc;
    if (plan_bytes < bound) return RLAP_E_BAD_ARG;
    if (!(flags & (RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED))) flags |= RLAP_PLAN_FORWARD | RLAP_PLAN_TRANSPOSED;
    return snapshot_call(h, [&] { return feature_build_bytes(N, Fin, flags); }, [&](void* base, size_t have, size_t need) -> int {
        if (h->poison >= 0) {   // debug: the plan must not depend on what the arena or the caller's buffer held
            RLAP_HIPCHK(hipMemsetAsync(base, h->poison, need, h->stream));
            RLAP_HIPCHK(hipMemsetAsync(d_plan, h->poison, plan_bytes, h->stream));
        }
        const FeatureBuildArgs a{d_x, N, Fin, nnz, flags, d_plan, plan_bytes};
        FeatureReport rep;
        const int rc = feature_build_run(h->stream, base, have, a, h_desc, &rep);
        if (rc != RLAP_OK) *h_desc = rlap_feature_desc{};
        if (h_info) {
            h_info->nnz = rep.nnz;
            h_info->longest_forward = rep.longest[0]; h_info->longest_transposed = rep.longest[1];
            h_info->long_lists_forward = rep.long_lists[0]; h_info->long_lists_transposed = rep.long_lists[1];
            h_info->chunks_forward = rep.chunks[0]; h_info->chunks_transposed = rep.chunks[1];
            h_info->arena_bytes = (int64_t)need; h_info->host_syncs = rep.host_syncs;
        }
        return rc;
    });
}

int rlap_feature_plan_apply(rlap_handle h, const void* d_plan, const rlap_feature_desc* h_desc, int flags, const void* d_w,
                            const uint8_t* d_keep, int64_t K, int64_t Fout, void* d_out, rlap_feature_info* h_info) {
    if (h_info) *h_info = rlap_feature_info{};
    if (!h || !d_plan || !h_desc || !d_w || !d_out || Fout < 1) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_SPMM_TRANSPOSE | RLAP_SPMM_X_F32)) return RLAP_E_BAD_ARG;
    if (K < 1 || K > featlin::MAX_VIEWS || (!d_keep && K != 1)) return RLAP_E_BAD_ARG;
    const rlap_feature_desc d = *h_desc;
    // a descriptor that a successful build wrote: every part it names lies inside the bytes it reports
    if (d.magic != featlin::MAGIC || d.num_nodes < 1 || d.num_nodes >= featlin::MAX_DIM || d.in_features < 1 || d.in_features >= featlin::MAX_DIM ||
        d.nnz < 0 || d.nnz >= featlin::MAX_NNZ || (reinterpret_cast<uintptr_t>(d_plan) & 15))
        return RLAP_E_BAD_ARG;
    const bool t = (flags & RLAP_SPMM_TRANSPOSE) != 0;
    if (!(d.flags & (t ? RLAP_PLAN_TRANSPOSED : RLAP_PLAN_FORWARD))) return RLAP_E_BAD_ARG;
    if (!featlin::parts_inside(t ? d.in_features : d.num_nodes, d.nnz, t ? d.chunks_transposed : d.chunks_forward,
                               t ? d.off_transposed : d.off_forward, t ? d.dir_transposed : d.dir_forward,
                               t ? d.rec_transposed : d.rec_forward, d.nnz, d.plan_bytes))
        return RLAP_E_BAD_ARG;
    if (Fout > SPMM_MAX_F || K * d.num_nodes * Fout >= SPMM_MAX_ELEMS || d.in_features * Fout >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    const int64_t out_elems = t ? d.in_features * Fout : K * d.num_nodes * Fout;
    return snapshot_call(h, [&] { return feature_apply_bytes(d, K, Fout, flags, h->dbg_scr); }, [&](void* base, size_t have, size_t need) -> int {
        if (h->poison >= 0) {   // debug: the result must not depend on what the arena or the result buffer held
            RLAP_HIPCHK(hipMemsetAsync(base, h->poison, need, h->stream));
            RLAP_HIPCHK(hipMemsetAsync(d_out, h->poison, (size_t)out_elems * ((flags & RLAP_SPMM_X_F32) ? 4 : 8), h->stream));
        }
        const FeatureApplyArgs a{d_plan, &d, flags, d_w, d_keep, K, Fout, d_out, h->dbg_scr};
        const int rc = feature_apply_run(h->stream, base, have, a);
        if (h_info) {
            h_info->nnz = d.nnz; h_info->chunks_forward = d.chunks_forward; h_info->chunks_transposed = d.chunks_transposed;
            h_info->longest_forward = h_info->longest_transposed = h_info->long_lists_forward = h_info->long_lists_transposed = -1;
            h_info->arena_bytes = (int64_t)need; h_info->host_syncs = 0;
        }
        return rc;
    });
}

namespace {

// what both readout exports check, and what the host knows of the call without reading the table
int readout_check(rlap_handle h, const void* d_in, int64_t L, int64_t N, int64_t F, const int64_t* d_node_ptr, int64_t G, int flags,
                  void* d_out, rlap_readout_info* h_info) {
    if (h_info) *h_info = rlap_readout_info{};
    if (!h || !d_node_ptr || L < 0 || N < 0 || F < 1 || G < 1) return RLAP_E_BAD_ARG;
    if (flags & ~(RLAP_READOUT_MEAN | RLAP_READOUT_X_F32)) return RLAP_E_BAD_ARG;
    if (F > SPMM_MAX_F || G >= SPMM_MAX_ELEMS || N >= SPMM_MAX_ELEMS || L >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    if (L * N >= SPMM_MAX_ELEMS || L * N * F >= SPMM_MAX_ELEMS || L * G >= SPMM_MAX_ELEMS || L * G * F >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    if ((L * N * F > 0 && !d_in) || (L * G * F > 0 && !d_out)) return RLAP_E_BAD_ARG;   // (either of them is x or y)
    if (h_info) {
        h_info->rows = N; h_info->graphs = G;
        h_info->chunks = G == 1 ? spmm::num_chunks(N) : readout::chunk_bound(N, G);
        h_info->chunked_graphs = G == 1 ? (N > spmm::CHUNK ? 1 : 0) : readout::chunked_bound(N, G);
    }
    return RLAP_OK;
}

}  // namespace

int rlap_graph_readout(rlap_handle h, const void* d_x, int64_t L, int64_t num_nodes, int64_t F, const int64_t* d_node_ptr, int64_t G,
                       int flags, void* d_y, rlap_readout_info* h_info) {
    if (const int rc = readout_check(h, d_x, L, num_nodes, F, d_node_ptr, G, flags, d_y, h_info)) return rc;
    const ReadoutArgs a{d_x, L, num_nodes, F, d_node_ptr, G, flags, d_y};
    return poisoned_call(h, [&] { return readout_bytes(L, num_nodes, F, G); }, {{d_y, (size_t)(L * G * F) * ((flags & RLAP_READOUT_X_F32) ? 4 : 8)}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return readout_run(h->stream, base, have, a); });
}

int rlap_graph_readout_backward(rlap_handle h, const void* d_gy, int64_t L, int64_t num_nodes, int64_t F, const int64_t* d_node_ptr,
                                int64_t G, int flags, void* d_gx, rlap_readout_info* h_info) {
    if (const int rc = readout_check(h, d_gx, L, num_nodes, F, d_node_ptr, G, flags, const_cast<void*>(d_gy), h_info)) return rc;
    const ReadoutArgs a{d_gy, L, num_nodes, F, d_node_ptr, G, flags, d_gx};
    // (no scratch: the gather reads the table itself)
    return poisoned_call(h, [&] { return (size_t)0; }, {{d_gx, (size_t)(L * num_nodes * F) * ((flags & RLAP_READOUT_X_F32) ? 4 : 8)}}, nullptr,
                         [&](void*, size_t) { return readout_backward_run(h->stream, a); });
}

namespace {

// what both InfoNCE exports check (their pointers come before this)
int infonce_check(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, rlap_infonce_info* h_info) {
    if (h_info) *h_info = rlap_infonce_info{};
    if (!h || !d_a || !d_b || N < 1 || F < 1 || !infonce::tau_ok(tau)) return RLAP_E_BAD_ARG;
    if (flags & ~RLAP_INFONCE_POSITIVE_RAW) return RLAP_E_BAD_ARG;
    if (F > infonce::MAX_F || N >= (int64_t)1 << 31) return RLAP_E_TOO_LARGE;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->parts = infonce::num_parts(N); }
    return RLAP_OK;
}

}  // namespace

int rlap_infonce(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, double* d_loss,
                 double* d_rows, double* d_z, rlap_infonce_info* h_info) {
    if (const int rc = infonce_check(h, d_a, d_b, N, F, tau, flags, h_info)) return rc;
    if (!d_loss || !d_rows || !d_z) return RLAP_E_BAD_ARG;
    InfonceArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.tau = tau; a.flags = flags; a.loss = d_loss; a.rows = d_rows; a.z = d_z;
    return poisoned_call(h, [&] { return infonce_bytes(N, F); }, {{d_loss, 8}, {d_rows, (size_t)N * 8}, {d_z, (size_t)N * 8}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return infonce_run(h->stream, base, have, a); });
}

int rlap_infonce_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags,
                          const double* d_z, const double* d_g, float* d_ga, float* d_gb, rlap_infonce_info* h_info) {
    if (const int rc = infonce_check(h, d_a, d_b, N, F, tau, flags, h_info)) return rc;
    if (!d_z || !d_g || !d_ga || !d_gb) return RLAP_E_BAD_ARG;
    InfonceArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.tau = tau; a.flags = flags; a.z_in = d_z; a.g = d_g; a.ga = d_ga; a.gb = d_gb;
    return poisoned_call(h, [&] { return infonce_backward_bytes(N, F); }, {{d_ga, (size_t)(N * F) * 4}, {d_gb, (size_t)(N * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return infonce_backward_run(h->stream, base, have, a); });
}

// the symmetric pair: the checks of rlap_infonce, its own info structure
int rlap_infonce_pair(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, double* d_loss,
                      double* d_rows, double* d_z, rlap_infonce_pair_info* h_info) {
    if (h_info) *h_info = rlap_infonce_pair_info{};
    if (const int rc = infonce_check(h, d_a, d_b, N, F, tau, flags, nullptr)) return rc;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->parts = infonce::pair_parts(N); h_info->groups = infonce::pair_groups(N); }
    if (!d_loss || !d_rows || !d_z) return RLAP_E_BAD_ARG;
    InfonceArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.tau = tau; a.flags = flags; a.loss = d_loss; a.rows = d_rows; a.z = d_z;
    return poisoned_call(h, [&] { return infonce_pair_bytes(N, F); }, {{d_loss, 8}, {d_rows, (size_t)N * 16}, {d_z, (size_t)N * 16}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return infonce_pair_run(h->stream, base, have, a); });
}

int rlap_infonce_pair_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags,
                               const double* d_z, const double* d_g, float* d_ga, float* d_gb, rlap_infonce_pair_info* h_info) {
    if (h_info) *h_info = rlap_infonce_pair_info{};
    if (const int rc = infonce_check(h, d_a, d_b, N, F, tau, flags, nullptr)) return rc;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->parts = infonce::pair_parts(N); h_info->groups = infonce::pair_groups(N); }
    if (!d_z || !d_g || !d_ga || !d_gb) return RLAP_E_BAD_ARG;
    InfonceArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.tau = tau; a.flags = flags; a.z_in = d_z; a.g = d_g; a.ga = d_ga; a.gb = d_gb;
    return poisoned_call(h, [&] { return infonce_pair_backward_bytes(N, F); }, {{d_ga, (size_t)(N * F) * 4}, {d_gb, (size_t)(N * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return infonce_pair_backward_run(h->stream, base, have, a); });
}

// intraview negatives: the four calls above with the variant behind `flags`; their checks first, then the variant's
static_assert(RLAP_INFONCE_INTRA_MASKED == infonce::INTRA_MASKED && RLAP_INFONCE_INTRA_ALL == infonce::INTRA_ALL, "the header's variants are the rule's");

int rlap_infonce_intra(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview,
                       double* d_loss, double* d_rows, double* d_z, rlap_infonce_info* h_info) {
    if (const int rc = infonce_check(h, d_a, d_b, N, F, tau, flags, h_info)) return rc;
    if (!d_loss || !d_rows || !d_z || !infonce::intra_ok(intraview)) return RLAP_E_BAD_ARG;
    InfonceArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.tau = tau; a.flags = flags; a.loss = d_loss; a.rows = d_rows; a.z = d_z; a.intraview = intraview;
    return poisoned_call(h, [&] { return infonce_bytes(N, F, intraview); }, {{d_loss, 8}, {d_rows, (size_t)N * 8}, {d_z, (size_t)N * 8}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return infonce_run(h->stream, base, have, a); });
}

int rlap_infonce_intra_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview,
                                const double* d_z, const double* d_g, float* d_ga, float* d_gb, rlap_infonce_info* h_info) {
    if (const int rc = infonce_check(h, d_a, d_b, N, F, tau, flags, h_info)) return rc;
    if (!d_z || !d_g || !d_ga || !d_gb || !infonce::intra_ok(intraview)) return RLAP_E_BAD_ARG;
    InfonceArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.tau = tau; a.flags = flags; a.z_in = d_z; a.g = d_g; a.ga = d_ga; a.gb = d_gb; a.intraview = intraview;
    return poisoned_call(h, [&] { return infonce_backward_bytes(N, F, intraview); }, {{d_ga, (size_t)(N * F) * 4}, {d_gb, (size_t)(N * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return infonce_backward_run(h->stream, base, have, a); });
}

int rlap_infonce_pair_intra(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview,
                            double* d_loss, double* d_rows, double* d_z, rlap_infonce_pair_info* h_info) {
    if (h_info) *h_info = rlap_infonce_pair_info{};
    if (const int rc = infonce_check(h, d_a, d_b, N, F, tau, flags, nullptr)) return rc;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->parts = infonce::pair_parts(N); h_info->groups = infonce::pair_groups(N); }
    if (!d_loss || !d_rows || !d_z || !infonce::intra_ok(intraview)) return RLAP_E_BAD_ARG;
    InfonceArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.tau = tau; a.flags = flags; a.loss = d_loss; a.rows = d_rows; a.z = d_z; a.intraview = intraview;
    return poisoned_call(h, [&] { return infonce_pair_bytes(N, F, intraview); }, {{d_loss, 8}, {d_rows, (size_t)N * 16}, {d_z, (size_t)N * 16}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return infonce_pair_run(h->stream, base, have, a); });
}

int rlap_infonce_pair_intra_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double tau, int flags, int intraview,
                                     const double* d_z, const double* d_g, float* d_ga, float* d_gb, rlap_infonce_pair_info* h_info) {
    if (h_info) *h_info = rlap_infonce_pair_info{};
    if (const int rc = infonce_check(h, d_a, d_b, N, F, tau, flags, nullptr)) return rc;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->parts = infonce::pair_parts(N); h_info->groups = infonce::pair_groups(N); }
    if (!d_z || !d_g || !d_ga || !d_gb || !infonce::intra_ok(intraview)) return RLAP_E_BAD_ARG;
    InfonceArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.tau = tau; a.flags = flags; a.z_in = d_z; a.g = d_g; a.ga = d_ga; a.gb = d_gb; a.intraview = intraview;
    return poisoned_call(h, [&] { return infonce_pair_backward_bytes(N, F, intraview); }, {{d_ga, (size_t)(N * F) * 4}, {d_gb, (size_t)(N * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return infonce_pair_backward_run(h->stream, base, have, a); });
}

namespace {

// what both CCA exports check (their pointers come before this)
int cca_check(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, int flags, rlap_cca_info* h_info) {
    if (h_info) *h_info = rlap_cca_info{};
    if (!h || !d_a || !d_b || N < 2 || F < 1 || F > cca::MAX_F || !cca::lambd_ok(lambd) || flags != 0) return RLAP_E_BAD_ARG;
    if (N >= (int64_t)1 << 31) return RLAP_E_TOO_LARGE;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->parts = cca::num_parts(N, F); }
    return RLAP_OK;
}

}  // namespace

int rlap_cca_loss(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, int flags, double* d_terms,
                  double* d_colstat, float* d_gram, rlap_cca_info* h_info) {
    if (const int rc = cca_check(h, d_a, d_b, N, F, lambd, flags, h_info)) return rc;
    if (!d_terms || !d_colstat || !d_gram) return RLAP_E_BAD_ARG;
    CcaArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.lambd = lambd; a.terms = d_terms; a.colstat = d_colstat; a.gram = d_gram;
    return poisoned_call(h, [&] { return cca_bytes(N, F); }, {{d_terms, 4 * 8}, {d_colstat, (size_t)(4 * F) * 8}, {d_gram, (size_t)(2 * F * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return cca_run(h->stream, base, have, a); });
}

int rlap_cca_loss_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, int flags,
                           const double* d_colstat, const float* d_gram, const double* d_g, float* d_ga, float* d_gb,
                           rlap_cca_info* h_info) {
    if (const int rc = cca_check(h, d_a, d_b, N, F, lambd, flags, h_info)) return rc;
    if (!d_colstat || !d_gram || !d_g || !d_ga || !d_gb) return RLAP_E_BAD_ARG;
    CcaArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.lambd = lambd; a.colstat_in = d_colstat; a.gram_in = d_gram; a.g = d_g; a.ga = d_ga; a.gb = d_gb;
    return poisoned_call(h, [&] { return cca_backward_bytes(N, F); }, {{d_ga, (size_t)(N * F) * 4}, {d_gb, (size_t)(N * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return cca_backward_run(h->stream, base, have, a); });
}

static_assert(RLAP_BT_NO_STANDARDIZE == bt::NO_STANDARDIZE, "the header's flag is the rule's");

namespace {

// what both Barlow Twins exports check (their pointers come before this)
int bt_check(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, double eps, int flags, rlap_bt_info* h_info) {
    if (h_info) *h_info = rlap_bt_info{};
    if (!h || !d_a || !d_b || N < 2 || F < 1 || F > bt::MAX_F || !bt::lambd_ok(lambd) || !bt::eps_ok(eps) || !bt::flags_ok(flags)) return RLAP_E_BAD_ARG;
    if (N >= (int64_t)1 << 31) return RLAP_E_TOO_LARGE;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->parts = bt::num_parts(N, F); }
    return RLAP_OK;
}

}  // namespace

int rlap_bt_loss(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, double eps, int flags,
                 double* d_terms, double* d_colstat, float* d_cross, rlap_bt_info* h_info) {
    if (const int rc = bt_check(h, d_a, d_b, N, F, lambd, eps, flags, h_info)) return rc;
    const bool plain = (flags & bt::NO_STANDARDIZE) != 0;
    if (!d_terms || (!d_colstat && !plain) || !d_cross) return RLAP_E_BAD_ARG;
    BtArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.lambd = lambd; a.eps = eps; a.flags = flags; a.terms = d_terms; a.colstat = d_colstat; a.cross = d_cross;
    return poisoned_call(h, [&] { return bt_bytes(N, F); }, {{d_terms, 3 * 8}, {plain ? nullptr : d_colstat, (size_t)(4 * F) * 8}, {d_cross, (size_t)(F * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return bt_run(h->stream, base, have, a); });
}

int rlap_bt_loss_backward(rlap_handle h, const float* d_a, const float* d_b, int64_t N, int64_t F, double lambd, double eps, int flags,
                          const double* d_colstat, const float* d_cross, const double* d_g, float* d_ga, float* d_gb,
                          rlap_bt_info* h_info) {
    if (const int rc = bt_check(h, d_a, d_b, N, F, lambd, eps, flags, h_info)) return rc;
    if ((!d_colstat && !(flags & bt::NO_STANDARDIZE)) || !d_cross || !d_g || !d_ga || !d_gb) return RLAP_E_BAD_ARG;
    BtArgs a{};
    a.a = d_a; a.b = d_b; a.N = N; a.F = F; a.lambd = lambd; a.eps = eps; a.flags = flags; a.colstat_in = d_colstat; a.cross_in = d_cross;
    a.g = d_g; a.ga = d_ga; a.gb = d_gb;
    return poisoned_call(h, [&] { return bt_backward_bytes(N, F); }, {{d_ga, (size_t)(N * F) * 4}, {d_gb, (size_t)(N * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return bt_backward_run(h->stream, base, have, a); });
}

static_assert(RLAP_LINEAR_WEIGHT_OUT_IN == linear::WEIGHT_OUT_IN && RLAP_LINEAR_ACT_NONE == linear::ACT_NONE &&
                  RLAP_LINEAR_ACT_RELU == linear::ACT_RELU && RLAP_LINEAR_ACT_ELU == linear::ACT_ELU, "the header's flag and activations are the rule's");

namespace {

// what both dense-layer exports check (their pointers come before this)
int linear_check(rlap_handle h, int64_t M, int64_t Fin, int64_t Fout, int act, double alpha, int flags, rlap_linear_info* h_info) {
    if (h_info) *h_info = rlap_linear_info{};
    if (!h || M < 1 || !linear::features_ok(Fin) || !linear::features_ok(Fout) || !linear::act_ok(act) || !linear::alpha_ok(alpha) ||
        !linear::flags_ok(flags))
        return RLAP_E_BAD_ARG;
    if (!linear::rows_ok(M)) return RLAP_E_TOO_LARGE;
    if (h_info) { h_info->rows = M; h_info->fin = Fin; h_info->fout = Fout; h_info->parts = linear::num_parts(M, Fin, Fout); }
    return RLAP_OK;
}

}  // namespace

int rlap_linear_act(rlap_handle h, const float* d_x, int64_t M, int64_t Fin, int64_t Fout, const float* d_w, const float* d_b, int act,
                    double alpha, int flags, float* d_y, rlap_linear_info* h_info) {
    if (const int rc = linear_check(h, M, Fin, Fout, act, alpha, flags, h_info)) return rc;
    if (!d_x || !d_w || !d_y) { if (h_info) *h_info = rlap_linear_info{}; return RLAP_E_BAD_ARG; }
    LinearArgs a{};
    a.x = d_x; a.w = d_w; a.b = d_b; a.M = M; a.Fin = Fin; a.Fout = Fout; a.act = act; a.alpha = alpha; a.flags = flags; a.y = d_y;
    return poisoned_call(h, [&] { return linear_bytes(M, Fin, Fout); }, {{d_y, (size_t)(M * Fout) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return linear_run(h->stream, base, have, a); });
}

int rlap_linear_act_backward(rlap_handle h, const float* d_x, const float* d_w, const float* d_y, const float* d_gy, int64_t M, int64_t Fin,
                             int64_t Fout, int act, double alpha, int flags, float* d_gx, float* d_gw, float* d_gb,
                             rlap_linear_info* h_info) {
    if (const int rc = linear_check(h, M, Fin, Fout, act, alpha, flags, h_info)) return rc;
    if (!d_x || !d_w || !d_y || !d_gy) { if (h_info) *h_info = rlap_linear_info{}; return RLAP_E_BAD_ARG; }
    LinearArgs a{};
    a.x = d_x; a.w = d_w; a.M = M; a.Fin = Fin; a.Fout = Fout; a.act = act; a.alpha = alpha; a.flags = flags;
    a.y_in = d_y; a.gy = d_gy; a.gx = d_gx; a.gw = d_gw; a.gb = d_gb;
    return poisoned_call(h, [&] { return linear_backward_bytes(M, Fin, Fout, d_gx != nullptr, d_gw != nullptr, d_gb != nullptr); },
                         {{d_gx, (size_t)(M * Fin) * 4}, {d_gw, (size_t)(Fin * Fout) * 4}, {d_gb, (size_t)Fout * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) { return linear_backward_run(h->stream, base, have, a); });
}

namespace {

// what the four graph-to-local exports check (their result pointers come before this)
int g2l_check(rlap_handle h, const float* d_h, const float* d_g, int64_t N, int64_t F, const int64_t* d_node_ptr, int64_t G, int flags,
              rlap_g2l_info* h_info) {
    if (h_info) *h_info = rlap_g2l_info{};
    if (!h || !d_h || !d_g || !d_node_ptr || N < 1 || F < 1 || G < 1 || flags != 0) return RLAP_E_BAD_ARG;
    if (F > g2l::MAX_F || N >= (int64_t)1 << 31 || G >= (int64_t)1 << 31) return RLAP_E_TOO_LARGE;
    if (h_info) { h_info->rows = N; h_info->graphs = G; h_info->features = F; h_info->parts = g2l::num_parts(N, G, F); }
    return RLAP_OK;
}

// one of the four calls on the checked path; `outs` are the result buffers a poisoned run fills first
int g2l_call(rlap_handle h, int call, const G2lArgs& a, rlap_g2l_info* h_info, PoisonList outs) {
    return poisoned_call(h, [&] { return g2l_bytes(call, a.N, a.G, a.F); }, outs, h_info ? &h_info->arena_bytes : nullptr,
                         [&](void* base, size_t have) { return g2l_run(call, h->stream, base, have, a); });
}

}  // namespace

int rlap_g2l_jsd(rlap_handle h, const float* d_h, const float* d_neg, const float* d_g, int64_t N, int64_t F, const int64_t* d_node_ptr,
                 int64_t G, int flags, double* d_loss, double* d_rows, rlap_g2l_info* h_info) {
    if (const int rc = g2l_check(h, d_h, d_g, N, F, d_node_ptr, G, flags, h_info)) return rc;
    if (!d_loss || !d_rows || (G == 1) != (d_neg != nullptr)) { if (h_info) *h_info = rlap_g2l_info{}; return RLAP_E_BAD_ARG; }
    G2lArgs a{};
    a.h = d_h; a.neg = d_neg; a.g = d_g; a.N = N; a.F = F; a.node_ptr = d_node_ptr; a.G = G; a.loss = d_loss; a.rows = d_rows;
    return g2l_call(h, g2l::JSD_FORWARD, a, h_info, {{d_loss, 8}, {d_rows, (size_t)(2 * N) * 8}});
}

int rlap_g2l_jsd_backward(rlap_handle h, const float* d_h, const float* d_neg, const float* d_g, int64_t N, int64_t F,
                          const int64_t* d_node_ptr, int64_t G, int flags, const double* d_gup, float* d_gh, float* d_gneg, float* d_gg,
                          rlap_g2l_info* h_info) {
    if (const int rc = g2l_check(h, d_h, d_g, N, F, d_node_ptr, G, flags, h_info)) return rc;
    if (!d_gup || !d_gh || !d_gg || (G == 1) != (d_neg != nullptr) || (G == 1) != (d_gneg != nullptr)) {
        if (h_info) *h_info = rlap_g2l_info{};
        return RLAP_E_BAD_ARG;
    }
    G2lArgs a{};
    a.h = d_h; a.neg = d_neg; a.g = d_g; a.N = N; a.F = F; a.node_ptr = d_node_ptr; a.G = G; a.gup = d_gup; a.gh = d_gh; a.gneg = d_gneg; a.gg = d_gg;
    return g2l_call(h, g2l::JSD_BACKWARD, a, h_info, {{d_gh, (size_t)(N * F) * 4}, {d_gneg, (size_t)(N * F) * 4}, {d_gg, (size_t)(G * F) * 4}});
}

int rlap_g2l_bootstrap(rlap_handle h, const float* d_h, const float* d_g, int64_t N, int64_t F, const int64_t* d_node_ptr, int64_t G,
                       int flags, double* d_loss, double* d_rows, rlap_g2l_info* h_info) {
    if (const int rc = g2l_check(h, d_h, d_g, N, F, d_node_ptr, G, flags, h_info)) return rc;
    if (!d_loss || !d_rows) { if (h_info) *h_info = rlap_g2l_info{}; return RLAP_E_BAD_ARG; }
    G2lArgs a{};
    a.h = d_h; a.g = d_g; a.N = N; a.F = F; a.node_ptr = d_node_ptr; a.G = G; a.loss = d_loss; a.rows = d_rows;
    return g2l_call(h, g2l::BOOT_FORWARD, a, h_info, {{d_loss, 8}, {d_rows, (size_t)N * 8}});
}

int rlap_g2l_bootstrap_backward(rlap_handle h, const float* d_h, const float* d_g, int64_t N, int64_t F, const int64_t* d_node_ptr,
                                int64_t G, int flags, const double* d_gup, float* d_gh, rlap_g2l_info* h_info) {
    if (const int rc = g2l_check(h, d_h, d_g, N, F, d_node_ptr, G, flags, h_info)) return rc;
    if (!d_gup || !d_gh) { if (h_info) *h_info = rlap_g2l_info{}; return RLAP_E_BAD_ARG; }
    G2lArgs a{};
    a.h = d_h; a.g = d_g; a.N = N; a.F = F; a.node_ptr = d_node_ptr; a.G = G; a.gup = d_gup; a.gh = d_gh;
    return g2l_call(h, g2l::BOOT_BACKWARD, a, h_info, {{d_gh, (size_t)(N * F) * 4}});
}

namespace {

// what both probe exports check on the host; the lists' contents and the labels are checked by the kernels (the status word)
int probe_check(rlap_handle h, const ProbeArgs& a, int lists, bool train, rlap_probe_info* h_info) {
    if (h_info) *h_info = rlap_probe_info{};
    auto fail = [&](int rc, int detail) { if (h_info) h_info->detail = detail; return rc; };
    if (!h || !a.x || !a.y || !a.w0 || !a.b0 || !a.scores || !a.confusion || !a.status) return fail(RLAP_E_BAD_ARG, probe::DETAIL_POINTER);
    if (train ? (!a.w || !a.b || !a.best) : !a.pred) return fail(RLAP_E_BAD_ARG, probe::DETAIL_POINTER);
    if (a.N < 1 || a.F < 1 || a.C < 2 || a.R < 1 || a.ldx < a.F) return fail(RLAP_E_BAD_ARG, probe::DETAIL_SHAPE);
    if (a.F > probe::MAX_F || a.C > probe::MAX_C || a.R > probe::MAX_RUNS || a.N >= (int64_t)1 << 31) return fail(RLAP_E_TOO_LARGE, probe::DETAIL_SHAPE);
    for (int s = 0; s < lists; ++s)
        if (!a.idx[s] || !probe_lists_ok(a.hptr[s], a.R)) return fail(RLAP_E_BAD_ARG, probe::DETAIL_LIST);
    if (train) {
        if (a.epochs < 1 || a.test_interval < 1 || (a.select != probe::SELECT_SCRIPTS && a.select != probe::SELECT_CCA))
            return fail(RLAP_E_BAD_ARG, probe::DETAIL_PARAM);
        if (!probe::finite_ok(a.lr) || !probe::finite_ok(a.wd) || a.wd < 0.0 || !(a.beta1 >= 0.0 && a.beta1 < 1.0) ||
            !(a.beta2 >= 0.0 && a.beta2 < 1.0) || !probe::finite_ok(a.eps) || !(a.eps > 0.0))
            return fail(RLAP_E_BAD_ARG, probe::DETAIL_PARAM);
    }
    if (h_info) h_info->runs = a.R;
    return RLAP_OK;
}

}  // namespace

int rlap_linear_probe(rlap_handle h, const float* d_x, int64_t N, int64_t F, int64_t ldx, const int64_t* d_y, int64_t C, int64_t R,
                      const int64_t* d_train, const int64_t* h_train_ptr, const int64_t* d_valid, const int64_t* h_valid_ptr,
                      const int64_t* d_test, const int64_t* h_test_ptr, int64_t epochs, double lr, double weight_decay,
                      int64_t test_interval, int select, double beta1, double beta2, double eps, const float* d_weight0,
                      const float* d_bias0, float* d_weight, float* d_bias, double* d_scores, int64_t* d_best, int64_t* d_confusion,
                      int32_t* d_status, rlap_probe_info* h_info) {
    ProbeArgs a{};
    a.x = d_x; a.N = N; a.F = F; a.ldx = ldx; a.y = d_y; a.C = C; a.R = R;
    a.idx[0] = d_train; a.hptr[0] = h_train_ptr; a.idx[1] = d_valid; a.hptr[1] = h_valid_ptr; a.idx[2] = d_test; a.hptr[2] = h_test_ptr;
    a.epochs = epochs; a.test_interval = test_interval; a.select = select; a.lr = lr; a.wd = weight_decay; a.beta1 = beta1; a.beta2 = beta2;
    a.eps = eps; a.w0 = d_weight0; a.b0 = d_bias0; a.w = d_weight; a.b = d_bias; a.scores = d_scores; a.best = d_best;
    a.confusion = d_confusion; a.status = d_status;
    if (const int rc = probe_check(h, a, 3, true, h_info)) return rc;
    // (parameters that are trained in place are inputs: not poisoned)
    return poisoned_call(h, [&] { return probe_bytes(a); },
                         {{d_weight != d_weight0 ? d_weight : nullptr, (size_t)(R * C * F) * 4}, {d_bias != d_bias0 ? d_bias : nullptr, (size_t)(R * C) * 4},
                          {d_scores, (size_t)(R * 4) * 8}, {d_best, (size_t)(R * 2) * 8}, {d_confusion, (size_t)(R * 2 * C * C) * 8}, {d_status, 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) {
        int64_t parts = 0, launches = 0;
        const int rc = probe_run(h->stream, base, have, a, &parts, &launches);
        if (h_info) { h_info->parts = parts; h_info->launches = launches; }
        return rc;
    });
}

int rlap_probe_scores(rlap_handle h, const float* d_x, int64_t N, int64_t F, int64_t ldx, const int64_t* d_y, int64_t C, int64_t R,
                      const int64_t* d_index, const int64_t* h_ptr, const float* d_weight, const float* d_bias, int64_t* d_pred,
                      int64_t* d_confusion, double* d_scores, int32_t* d_status, rlap_probe_info* h_info) {
    ProbeArgs a{};
    a.x = d_x; a.N = N; a.F = F; a.ldx = ldx; a.y = d_y; a.C = C; a.R = R; a.idx[0] = d_index; a.hptr[0] = h_ptr;
    a.w0 = d_weight; a.b0 = d_bias; a.pred = d_pred; a.confusion = d_confusion; a.scores = d_scores; a.status = d_status;
    if (const int rc = probe_check(h, a, 1, false, h_info)) return rc;
    return poisoned_call(h, [&] { return scores_bytes(a); },
                         {{d_pred, (size_t)h_ptr[R] * 8}, {d_confusion, (size_t)(R * C * C) * 8}, {d_scores, (size_t)(R * 3) * 8}, {d_status, 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) {
        int64_t launches = 0;
        const int rc = scores_run(h->stream, base, have, a, &launches);
        if (h_info) { h_info->parts = 1; h_info->launches = launches; }
        return rc;
    });
}

namespace {

// what both norm exports check (their own pointers come behind this), and what the host knows of the call
int norm_check(rlap_handle h, const float* d_x, int64_t L, int64_t N, int64_t F, const float* d_slope, const float* d_rm, const float* d_rv,
               double momentum, double eps, int flags, const double* d_stat, rlap_norm_info* h_info) {
    if (h_info) *h_info = rlap_norm_info{};
    if (!h || !d_x || !norm::args_ok(L, N, F, flags, d_slope != nullptr, d_rm && d_rv, eps, momentum)) return RLAP_E_BAD_ARG;
    if (!(flags & RLAP_NORM_EVAL) && !d_stat) return RLAP_E_BAD_ARG;
    if (L >= SPMM_MAX_ELEMS || N >= SPMM_MAX_ELEMS || L * N >= SPMM_MAX_ELEMS || L * N * F >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->layers = L; h_info->chunks = spmm::num_chunks(N); }
    return RLAP_OK;
}

void norm_report(rlap_norm_info* h_info, const NormReport& rep) {
    if (h_info) { h_info->vec = rep.vec; h_info->launches = rep.launches; h_info->chunks = rep.chunks; }
}

}  // namespace

int rlap_batch_norm(rlap_handle h, const float* d_x, int64_t L, int64_t N, int64_t F, const float* d_weight, const float* d_bias,
                    const float* d_slope, float* d_running_mean, float* d_running_var, double momentum, double eps, int flags,
                    float* d_y, double* d_stat, rlap_norm_info* h_info) {
    if (const int rc = norm_check(h, d_x, L, N, F, d_slope, d_running_mean, d_running_var, momentum, eps, flags, d_stat, h_info)) return rc;
    if (!d_y) return RLAP_E_BAD_ARG;
    const bool eval = (flags & RLAP_NORM_EVAL) != 0;
    NormArgs a{};
    a.x = d_x; a.L = L; a.N = N; a.F = F; a.weight = d_weight; a.bias = d_bias; a.slope = d_slope;
    a.running_mean = d_running_mean; a.running_var = d_running_var;
    a.upd_mean = eval ? nullptr : d_running_mean; a.upd_var = eval ? nullptr : d_running_var;
    a.momentum = momentum; a.eps = eps; a.flags = flags; a.out = d_y; a.stat = d_stat;
    // (the running buffers of a training call are inputs as well: not poisoned)
    return poisoned_call(h, [&] { return norm_bytes(a, false); }, {{d_y, (size_t)(L * N * F) * 4}, {eval ? nullptr : d_stat, (size_t)(L * 3 * F) * 8}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) {
        NormReport rep{};
        const int rc = norm_run(h->stream, base, have, a, &rep);
        if (rc == RLAP_OK) norm_report(h_info, rep);
        return rc;
    });
}

int rlap_batch_norm_backward(rlap_handle h, const float* d_x, const float* d_gy, int64_t L, int64_t N, int64_t F, const float* d_weight,
                    const float* d_bias, const float* d_slope, const float* d_running_mean, const float* d_running_var, double eps,
                    int flags, const double* d_stat, float* d_gx, float* d_gweight, float* d_gbias, float* d_gslope,
                    rlap_norm_info* h_info) {
    if (const int rc = norm_check(h, d_x, L, N, F, d_slope, d_running_mean, d_running_var, 0.0, eps, flags, d_stat, h_info)) return rc;
    if (!d_gy) return RLAP_E_BAD_ARG;
    NormArgs a{};
    a.x = d_x; a.gy = d_gy; a.L = L; a.N = N; a.F = F; a.weight = d_weight; a.bias = d_bias; a.slope = d_slope;
    a.running_mean = d_running_mean; a.running_var = d_running_var; a.eps = eps; a.flags = flags; a.out = d_gx;
    a.stat = const_cast<double*>(d_stat);
    a.gweight = d_gweight; a.gbias = d_gbias; a.gslope = (flags & RLAP_NORM_POST_PRELU) ? d_gslope : nullptr;
    const size_t slope_bytes = (size_t)((flags & RLAP_NORM_SLOPE_PER_CHANNEL) ? F : 1) * 4;
    return poisoned_call(h, [&] { return norm_bytes(a, true); },
                         {{d_gx, (size_t)(L * N * F) * 4}, {d_gweight, (size_t)F * 4}, {d_gbias, (size_t)F * 4}, {a.gslope, slope_bytes}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) {
        NormReport rep{};
        const int rc = norm_backward_run(h->stream, base, have, a, &rep);
        if (rc == RLAP_OK) norm_report(h_info, rep);
        return rc;
    });
}

namespace {

// what both row-pass exports check (their own pointers come behind this), and what the host knows of the call
int rowops_check(rlap_handle h, const float* d_x, int64_t L, int64_t N, int64_t F, const float* d_slope, double p, int flags,
                 rlap_rowops_info* h_info) {
    if (h_info) *h_info = rlap_rowops_info{};
    if (!h || !d_x || !rowops::args_ok(L, N, F, flags, d_slope != nullptr, p)) return RLAP_E_BAD_ARG;
    if (L >= SPMM_MAX_ELEMS || N >= SPMM_MAX_ELEMS || L * N >= SPMM_MAX_ELEMS || L * N * F >= SPMM_MAX_ELEMS) return RLAP_E_TOO_LARGE;
    if (h_info) { h_info->rows = N; h_info->features = F; h_info->layers = L; h_info->chunks = spmm::num_chunks(N); }
    return RLAP_OK;
}

void rowops_report(rlap_rowops_info* h_info, const RowopsReport& rep) {
    if (h_info) { h_info->vec = rep.vec; h_info->launches = rep.launches; h_info->chunks = rep.chunks; h_info->instance = rep.instance; }
}

}  // namespace

int rlap_bias_act_dropout(rlap_handle h, const float* d_x, int64_t L, int64_t N, int64_t F, const float* d_bias, const float* d_slope,
                    double p, uint64_t seed, int flags, float* d_y, rlap_rowops_info* h_info) {
    if (const int rc = rowops_check(h, d_x, L, N, F, d_slope, p, flags, h_info)) return rc;
    if (!d_y) return RLAP_E_BAD_ARG;
    RowopsArgs a{};
    a.x = d_x; a.L = L; a.N = N; a.F = F; a.bias = d_bias; a.slope = d_slope; a.p = p; a.seed = seed; a.flags = flags; a.out = d_y;
    return poisoned_call(h, [&] { return rowops_bytes(a, false); }, {{d_y, (size_t)(L * N * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) {
        RowopsReport rep{};
        const int rc = rowops_run(h->stream, base, have, a, &rep);
        if (rc == RLAP_OK) rowops_report(h_info, rep);
        return rc;
    });
}

int rlap_bias_act_dropout_backward(rlap_handle h, const float* d_x, const float* d_gy, int64_t L, int64_t N, int64_t F,
                    const float* d_bias, const float* d_slope, double p, uint64_t seed, int flags, float* d_gx, float* d_gbias,
                    float* d_gslope, rlap_rowops_info* h_info) {
    if (const int rc = rowops_check(h, d_x, L, N, F, d_slope, p, flags, h_info)) return rc;
    if (!d_gy) return RLAP_E_BAD_ARG;
    RowopsArgs a{};
    a.x = d_x; a.gy = d_gy; a.L = L; a.N = N; a.F = F; a.bias = d_bias; a.slope = d_slope; a.p = p; a.seed = seed; a.flags = flags;
    a.out = d_gx; a.gbias = d_gbias; a.gslope = (flags & RLAP_ROW_ACT_PRELU) ? d_gslope : nullptr;
    const size_t slope_bytes = (size_t)((flags & RLAP_ROW_SLOPE_PER_CHANNEL) ? F : 1) * 4;
    return poisoned_call(h, [&] { return rowops_bytes(a, true); },
                         {{d_gx, (size_t)(L * N * F) * 4}, {d_gbias, (size_t)F * 4}, {a.gslope, slope_bytes}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) {
        RowopsReport rep{};
        const int rc = rowops_backward_run(h->stream, base, have, a, &rep);
        if (rc == RLAP_OK) rowops_report(h_info, rep);
        return rc;
    });
}

int rlap_layer_norm(rlap_handle h, const float* d_x, int64_t L, int64_t N, int64_t F, const float* d_weight, const float* d_bias,
                    const float* d_slope, double eps, double p, uint64_t seed, int flags, float* d_y, rlap_rowops_info* h_info) {
    if (const int rc = rowops_check(h, d_x, L, N, F, d_slope, p, flags, h_info)) return rc;
    if (!d_y || !norm::eps_ok(eps)) return RLAP_E_BAD_ARG;
    RowopsArgs a{};
    a.x = d_x; a.L = L; a.N = N; a.F = F; a.weight = d_weight; a.bias = d_bias; a.slope = d_slope; a.eps = eps; a.p = p; a.seed = seed;
    a.flags = flags; a.out = d_y;
    return poisoned_call(h, [&] { return ln_bytes(a, false); }, {{d_y, (size_t)(L * N * F) * 4}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) {
        RowopsReport rep{};
        const int rc = ln_run(h->stream, base, have, a, &rep);
        if (rc == RLAP_OK) rowops_report(h_info, rep);
        return rc;
    });
}

int rlap_layer_norm_backward(rlap_handle h, const float* d_x, const float* d_gy, int64_t L, int64_t N, int64_t F, const float* d_weight,
                    const float* d_bias, const float* d_slope, double eps, double p, uint64_t seed, int flags, float* d_gx,
                    float* d_gweight, float* d_gbias, float* d_gslope, rlap_rowops_info* h_info) {
    if (const int rc = rowops_check(h, d_x, L, N, F, d_slope, p, flags, h_info)) return rc;
    if (!d_gy || !norm::eps_ok(eps)) return RLAP_E_BAD_ARG;
    RowopsArgs a{};
    a.x = d_x; a.gy = d_gy; a.L = L; a.N = N; a.F = F; a.weight = d_weight; a.bias = d_bias; a.slope = d_slope; a.eps = eps; a.p = p;
    a.seed = seed; a.flags = flags; a.out = d_gx; a.gweight = d_gweight; a.gbias = d_gbias;
    a.gslope = (flags & RLAP_ROW_ACT_PRELU) ? d_gslope : nullptr;
    const size_t slope_bytes = (size_t)((flags & RLAP_ROW_SLOPE_PER_CHANNEL) ? F : 1) * 4;
    return poisoned_call(h, [&] { return ln_bytes(a, true); },
                         {{d_gx, (size_t)(L * N * F) * 4}, {d_gweight, (size_t)F * 4}, {d_gbias, (size_t)F * 4}, {a.gslope, slope_bytes}},
                         h_info ? &h_info->arena_bytes : nullptr, [&](void* base, size_t have) {
        RowopsReport rep{};
        const int rc = ln_backward_run(h->stream, base, have, a, &rep);
        if (rc == RLAP_OK) rowops_report(h_info, rep);
        return rc;
    });
}

int rlap_debug_set_limits(rlap_handle h, double pool_factor, double log_factor, int64_t rng_len, int64_t scratch_entries) {
    if (!h) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->dbg_pool = pool_factor; h->dbg_log = log_factor; h->dbg_rng = rng_len; h->dbg_scr = scratch_entries;
    return RLAP_OK;
}

int rlap_debug_set_flow_limits(rlap_handle h, int64_t reorder_cap) {
    if (!h) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->dbg_ro_cap = reorder_cap;
    return RLAP_OK;
}

int rlap_debug_set_poison(rlap_handle h, int byte) {
    if (!h) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->poison = byte < 0 ? -1 : (byte & 0xFF);
    return RLAP_OK;
}

int rlap_debug_set_jitter(rlap_handle h, int quarter_us) {
    if (!h) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    h->jitter = std::max(0, std::min(64, quarter_us));
    return RLAP_OK;
}

int rlap_rng_uniforms(rlap_handle h, int64_t count, double* d_out) {
    if (!h || count < 0) return RLAP_E_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    DeviceGuard dg(h->device);
    int rc = ensure_rng(h, count);
    if (rc) return rc;
    RLAP_HIPCHK(hipMemcpyAsync(d_out, h->rng_ptr, sizeof(double) * (size_t)count, hipMemcpyDeviceToDevice, h->stream));
    RLAP_HIPCHK(hipStreamSynchronize(h->stream));
    return RLAP_OK;
}

int rlap_debug_wave_sort(rlap_handle h, const double* d_keys, const int32_t* d_offs, int32_t narr, int32_t desc, int32_t* d_perm_out) {
    if (!h || narr < 0) return RLAP_E_BAD_ARG;
    if (narr == 0) return RLAP_OK;
    if (desc & 32) {   // the dataflow kernel's long-column sort (rlap_flow.hip)
        int32_t total = 0;
        RLAP_HIPCHK(hipMemcpy(&total, d_offs + narr, 4, hipMemcpyDeviceToHost));
        DevBuf scr;
        ENSURE(scr, 32 * (size_t)std::max(total, 1) + 64 * (size_t)narr + 256);
        launch_debug_flow_sort(h->stream, d_keys, d_offs, narr, desc, d_perm_out, scr.as<char>());
        RLAP_HIPCHK(hipGetLastError());
        RLAP_HIPCHK(hipStreamSynchronize(h->stream));
        scr.release();
        return RLAP_OK;
    }
    hipLaunchKernelGGL(k_debug_wave_sort, dim3((unsigned)std::min<int32_t>(narr, 2048)), dim3(64), 0, h->stream, d_keys, d_offs, narr, desc, d_perm_out);
    RLAP_HIPCHK(hipGetLastError());
    RLAP_HIPCHK(hipStreamSynchronize(h->stream));
    return RLAP_OK;
}

// networkx-style BA generator (repeated-endpoint list), own xorshift RNG.
int64_t rlap_util_ba_graph(int64_t n, int64_t m, uint64_t seed, int64_t* h_row, int64_t* h_col) {
    if (n <= m || m < 1) return 0;
    int64_t und = m * (n - m);
    if (!h_row || !h_col) return 2 * und;
    std::vector<int32_t> rep;
    rep.reserve((size_t)(2 * und));
    std::vector<int32_t> targets((size_t)m);
    for (int64_t i = 0; i < m; ++i) targets[i] = (int32_t)i;
    std::vector<uint64_t> keys;
    keys.reserve((size_t)(2 * und));
    uint64_t sst = seed * 0x9E3779B97F4A7C15ull + 0x1234567ull;
    auto next = [&]() { sst = mix64(sst); return sst; };
    std::vector<int32_t> mark((size_t)n, -1);
    for (int64_t i = m; i < n; ++i) {
        for (int64_t j = 0; j < m; ++j) {
            int64_t tg = targets[j];
            keys.push_back(((uint64_t)tg << 32) | (uint64_t)i);  // (col=tg,row=i)
            keys.push_back(((uint64_t)i << 32) | (uint64_t)tg);
            rep.push_back((int32_t)tg);
        }
        for (int64_t j = 0; j < m; ++j) rep.push_back((int32_t)i);
        int64_t got = 0;
        while (got < m) {
            uint64_t r = next();
            int32_t cand = rep[(size_t)(((unsigned __int128)r * (unsigned __int128)rep.size()) >> 64)];
            if (mark[cand] != (int32_t)i) { mark[cand] = (int32_t)i; targets[got++] = cand; }
        }
    }
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    for (size_t k = 0; k < keys.size(); ++k) { h_col[k] = (int64_t)(keys[k] >> 32); h_row[k] = (int64_t)(keys[k] & 0xFFFFFFFFull); }
    return (int64_t)keys.size();
}

}  // extern "C"
