// rlap_edgeplan.hip -- propagation plans for rows in any order (rlap_edge_plan_build): the plan buffer of
// rlap_plan.hip -- the same layout, read by the same planned call -- built from a row table whose segments hold their rows in any
// order: a plain COO edge list, the (out, pptr) of rlap_snapshot_ppr, a subgraph result.  The order rules are rlap_edgeplan.h's.
// A translation unit of its own: no device function is shared with the elimination kernels, and rlap_plan.hip is not touched.
//
//   tables   rlap_gcn.hip's checked copies of ptr / node_ptr.
//   keys     one pass over the rows, two rows a lane (three 16-byte loads when sc is 16-byte aligned): the segment, both ids
//            checked (integral, inside the graph's range), the weight checked (weighted and normalised), the target slot key and
//            the source slot key, slot = layer * N + id; the loop rows counted.  A row that fails raises an error word and gets
//            key 0; every later kernel returns on a raised word.
//   sorts    rocPRIM's stable radix sort of (key, row) by target -- always: the degrees need it -- and by source (transposed),
//            over the bits the slots need; a pass over the sorted keys gives [lo, hi) of every slot and counts the lists.
//   degrees  16 lanes per slot walk the target's sorted range through perm, four rows in flight: rlap_edgeplan.h's rule; writes
//            dis[slot] and the loop's weight lw[slot] of EVERY slot (an empty list: the loop's weight alone).
//   count, scans, fill, directory   as rlap_plan.hip's, with lists through perm and blocks replaced by slots.  Every record's
//            position is checked against its list's [off[slot], off[slot + 1]) and against the m records the buffer holds.
//   One read-back of the error words, the counts and the last scan entries.  No LDS, no atomic on a float.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "../../include/rlap_hip.h"
#include "rlap_edgeplan.h"
#include "rlap_gcn.h"
#include "rlap_gcnmath.h"
#include "rlap_plan.h"
#include "rlap_spmm.h"

namespace rlap {
namespace {

constexpr int EP_THREADS = 256;
constexpr int64_t EP_MAX_GRID = 8192;                    // workgroups of a launch (the kernels stride over their tasks)
enum { CNT_LOOPS = 0, CNT_BLOCKS = 1, CNT_CHUNKED_F = 2, CNT_CHUNKED_T = 3, CNT_WORDS = 4 };

inline unsigned ep_blocks(int64_t n, int bs) { return capped_blocks(n, bs, EP_MAX_GRID); }

__device__ inline int64_t ep_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// what the build's kernels share (ptr / node_ptr are the checked copies)
struct Eb {
    const double* sc; int64_t m;
    const int64_t* ptr; int64_t S;
    const int64_t* node_ptr; int64_t G;
    int64_t N, slots;
    int weighted, loops, normalize;
    double fill;
    uint32_t* key[2];                         // [m] the slot of a row's target / source
    const uint32_t* skey[2]; const int32_t* perm[2];   // sorted keys and their rows
    int32_t* lo[2]; int32_t* hi[2];           // [slots] the positions of every slot among the sorted rows
    double* dis; double* lw;                  // [slots] deg^-1/2 and the weight of the slot's loop
    unsigned long long* cnt;                  // [CNT_WORDS]
    int32_t* err;
    // one direction
    int transpose;
    int32_t* kept; int32_t* nch;              // [slots + 1] entries that stay, chunks of a long list
    int64_t* off; const int64_t* choff;       // their exclusive scans
    plan::Record* rec; plan::ChunkRef* dir; int64_t dcap;
    double* loopc;                            // [slots] or nullptr (not this launch's to write)
};

__device__ inline bool eb_failed(const Eb& a) { return (a.err[COL_ERR_RANGE] | a.err[GCN_ERR_ARG]) != 0; }

__device__ inline bool eb_drop(const Eb& a) { return a.loops && a.m > 0 && a.cnt[CNT_LOOPS] != 0; }

// the list of `slot` in direction d: n positions of perm[d] from s on
__device__ inline void eb_list(const Eb& a, int d, int64_t slot, int64_t& s, int64_t& n) {
    s = ep_clamp(a.lo[d][slot], 0, a.m);
    n = ep_clamp(a.hi[d][slot], s, a.m) - s;
}

__device__ inline int64_t eb_row(const Eb& a, int d, int64_t pos) { return ep_clamp(a.perm[d][pos], 0, a.m - 1); }

// an id of graph range [lo, hi): integral and inside it (false for NaN)
__device__ inline bool eb_id_ok(double v, int64_t lo, int64_t hi) { return v >= (double)lo && v < (double)hi && v == floor(v); }

__device__ inline void eb_key(const Eb& a, int check, int64_t r, double vi, double vj, double w) {
    const int64_t s = seg_of(a.ptr, a.S, r);
    const int64_t layer = s / a.G, g = s - layer * a.G;
    const int64_t lo = a.node_ptr ? a.node_ptr[g] : 0, hi = a.node_ptr ? a.node_ptr[g + 1] : a.N;
    const bool ok = eb_id_ok(vi, lo, hi) && eb_id_ok(vj, lo, hi);
    if (!ok) atomicOr(&a.err[COL_ERR_RANGE], 1);
    if (check && !gcnmath::weight_ok(w)) atomicOr(&a.err[GCN_ERR_WEIGHT], 1);
    a.key[0][r] = ok ? (uint32_t)plan::slot_of(layer, a.N, (int64_t)vj) : 0u;
    a.key[1][r] = ok ? (uint32_t)plan::slot_of(layer, a.N, (int64_t)vi) : 0u;
    if (a.loops && ok && vi == vj) atomicAdd(&a.cnt[CNT_LOOPS], 1ull);
}

// the keys of two rows a lane; val[r] = r for the sorts
__global__ __launch_bounds__(EP_THREADS) void k_ep_keys(Eb a, int vec, int check, int32_t* __restrict__ val) {
    const int64_t pairs = (a.m + 1) / 2;
    for (int64_t p = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x; p < pairs; p += (int64_t)gridDim.x * EP_THREADS) {
        const int64_t r0 = 2 * p;
        const bool two = r0 + 1 < a.m;
        const double* __restrict__ in = a.sc + 3 * r0;
        double v[6] = {0.0, 0.0, 1.0, 0.0, 0.0, 1.0};
        if (vec && two) {   // (48 bytes a pair: the pair starts on a 16-byte boundary when sc does)
            const double2* __restrict__ s2 = reinterpret_cast<const double2*>(in);
            const double2 q0 = s2[0], q1 = s2[1], q2 = s2[2];
            v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y; v[4] = q2.x; v[5] = q2.y;
        } else {
            v[0] = in[0]; v[1] = in[1]; v[2] = in[2];
            if (two) { v[3] = in[3]; v[4] = in[4]; v[5] = in[5]; }
        }
        eb_key(a, check, r0, v[0], v[1], a.weighted ? v[2] : 1.0);
        val[r0] = (int32_t)r0;
        if (two) {
            eb_key(a, check, r0 + 1, v[3], v[4], a.weighted ? v[5] : 1.0);
            val[r0 + 1] = (int32_t)(r0 + 1);
        }
    }
}

// [lo[slot], hi[slot]) = the positions of the slot in the sorted keys of direction d (both zeroed before); forward: the lists
__global__ __launch_bounds__(EP_THREADS) void k_ep_bounds(Eb a, int d) {
    if (eb_failed(a)) return;
    const uint32_t* __restrict__ keys = a.skey[d];
    for (int64_t p = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x; p < a.m; p += (int64_t)gridDim.x * EP_THREADS) {
        const int64_t key = keys[p];
        if (key >= a.slots) continue;
        if (p == 0 || keys[p - 1] != key) {
            a.lo[d][key] = (int32_t)p;
            if (d == 0) atomicAdd(&a.cnt[CNT_BLOCKS], 1ull);
        }
        if (p == a.m - 1 || keys[p + 1] != key) a.hi[d][key] = (int32_t)(p + 1);
    }
}

// per slot: dis, the loop's weight.  16 lanes a slot; a lane takes the places place_of(turn, u, lane) of the target's list, four
// a turn: their rows' numbers first, then the rows, then the adds (a place past the end repeats the last one's loads and adds
// nothing).
__global__ __launch_bounds__(EP_THREADS) void k_ep_degree(Eb a) {
    if (eb_failed(a)) return;
    const int sub = threadIdx.x & (edgeplan::LANES - 1);
    const int64_t stride = (int64_t)gridDim.x * EP_THREADS / edgeplan::LANES;
    for (int64_t slot = ((int64_t)blockIdx.x * EP_THREADS + threadIdx.x) / edgeplan::LANES; slot < a.slots; slot += stride) {
        int64_t s, n;   // (whole groups share a slot: the butterflies below stay inside a group)
        eb_list(a, 0, slot, s, n);
        double acc[edgeplan::ACCS] = {0.0, 0.0, 0.0, 0.0};
        int64_t last = -1;   // place of the list's last loop row
        for (int64_t turn = 0; edgeplan::place_of(turn, 0, sub) < n; ++turn) {
            int64_t r[edgeplan::ACCS];
#pragma unroll
            for (int u = 0; u < edgeplan::ACCS; ++u) r[u] = eb_row(a, 0, s + std::min<int64_t>(edgeplan::place_of(turn, u, sub), n - 1));
            double vi[edgeplan::ACCS], vj[edgeplan::ACCS], w[edgeplan::ACCS];
#pragma unroll
            for (int u = 0; u < edgeplan::ACCS; ++u) {
                vi[u] = a.sc[3 * r[u]];
                vj[u] = a.sc[3 * r[u] + 1];
                w[u] = a.weighted ? a.sc[3 * r[u] + 2] : 1.0;
            }
#pragma unroll
            for (int u = 0; u < edgeplan::ACCS; ++u) {
                const int64_t k = edgeplan::place_of(turn, u, sub);
                if (k >= n) continue;
                if (a.loops && vi[u] == vj[u]) last = std::max(last, k);
                else acc[u] += w[u];
            }
        }
        double d = edgeplan::combine(acc);
#pragma unroll
        for (int o = edgeplan::LANES / 2; o > 0; o >>= 1) {
            d = edgeplan::meet(d, __shfl_xor(d, o));
            last = std::max<int64_t>(last, __shfl_xor(last, o));
        }
        if (sub != 0) continue;
        double w = a.fill;
        if (last >= 0) w = a.weighted ? a.sc[3 * eb_row(a, 0, s + last) + 2] : 1.0;
        a.dis[slot] = gcnmath::dis(edgeplan::finish(d, a.loops != 0, w));
        a.lw[slot] = w;
    }
}

// the record of row r of `layer`: the coefficient rlap_snapshot_gcn_norm gives it, and the id whose features the direction takes
__device__ inline plan::Record eb_record(const Eb& a, int64_t layer, int64_t r) {
    const int64_t i = ep_clamp((int64_t)a.sc[3 * r], 0, a.N - 1), j = ep_clamp((int64_t)a.sc[3 * r + 1], 0, a.N - 1);
    const double w = a.weighted ? a.sc[3 * r + 2] : 1.0;
    plan::Record e;
    e.c = a.normalize ? gcnmath::value(a.dis[plan::slot_of(layer, a.N, i)], w, a.dis[plan::slot_of(layer, a.N, j)]) : w;
    e.id = (int32_t)(a.transpose ? j : i);
    e.zero = 0;
    return e;
}

// per slot (and one entry behind the last): the entries of its list that stay, the chunks of a long list; the loop coefficient
__global__ __launch_bounds__(EP_THREADS) void k_ep_count(Eb a) {
    const bool ok = !eb_failed(a);
    const bool drop = eb_drop(a);
    const int d = a.transpose;
    for (int64_t slot = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x; slot <= a.slots; slot += (int64_t)gridDim.x * EP_THREADS) {
        int64_t kept = 0;
        if (ok && slot < a.slots) {
            int64_t s, n;
            eb_list(a, d, slot, s, n);
            kept = n;
            if (drop) {
                kept = 0;
                for (int64_t k = 0; k < n; ++k) {
                    const int64_t r = eb_row(a, d, s + k);
                    kept += a.sc[3 * r] == a.sc[3 * r + 1] ? 0 : 1;
                }
            }
        }
        const int64_t nc = plan::dir_chunks(kept);
        if (nc > 0) atomicAdd(&a.cnt[d ? CNT_CHUNKED_T : CNT_CHUNKED_F], 1ull);
        a.kept[slot] = (int32_t)kept;
        a.nch[slot] = (int32_t)nc;
        if (a.loopc && slot < a.slots) {   // (the loop of rlap_gcn.hip's k_gc_tail, as k_pl_count forms it)
            const double w = ok ? a.lw[slot] : a.fill;
            const double dd = ok ? a.dis[slot] : gcnmath::dis(a.fill);
            a.loopc[slot] = a.normalize ? gcnmath::value(dd, w, dd) : w;
        }
    }
}

// the records, one lane per sorted position; not for an input with dropped loop rows
__global__ __launch_bounds__(EP_THREADS) void k_ep_fill(Eb a) {
    if (eb_failed(a) || eb_drop(a)) return;
    const int d = a.transpose;
    for (int64_t p = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x; p < a.m; p += (int64_t)gridDim.x * EP_THREADS) {
        const int64_t slot = a.skey[d][p];
        if (slot >= a.slots) continue;
        const int64_t r = eb_row(a, d, p);
        const int64_t first = ep_clamp(a.lo[d][slot], 0, a.m);
        const int64_t at = plan::record_index(a.off[slot], a.off[slot + 1], plan::place_plain(first, p));
        if (at >= 0 && at < a.m) a.rec[at] = eb_record(a, slot / a.N, r);
    }
}

// the records of an input with dropped loop rows: one lane walks a list, counting
__global__ __launch_bounds__(EP_THREADS) void k_ep_fill_walk(Eb a) {
    if (eb_failed(a) || !eb_drop(a)) return;
    const int d = a.transpose;
    for (int64_t slot = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x; slot < a.slots; slot += (int64_t)gridDim.x * EP_THREADS) {
        int64_t s, n;
        eb_list(a, d, slot, s, n);
        int64_t place = 0;
        for (int64_t k = 0; k < n; ++k) {
            const int64_t r = eb_row(a, d, s + k);
            if (a.sc[3 * r] == a.sc[3 * r + 1]) continue;
            const int64_t at = plan::record_index(a.off[slot], a.off[slot + 1], place++);
            if (at >= 0 && at < a.m) a.rec[at] = eb_record(a, slot / a.N, r);
        }
    }
}

// the directory: the (slot, chunk) of every chunk number
__global__ __launch_bounds__(EP_THREADS) void k_ep_dir(Eb a) {
    if (eb_failed(a)) return;
    for (int64_t slot = (int64_t)blockIdx.x * EP_THREADS + threadIdx.x; slot < a.slots; slot += (int64_t)gridDim.x * EP_THREADS) {
        if (a.nch[slot] == 0) continue;
        plan::dir_write(slot, a.kept[slot], a.choff[slot], a.dcap, [&](int64_t q, plan::ChunkRef c) { a.dir[q] = c; });
    }
}

struct Bufs {
    int32_t* err;
    unsigned long long* cnt;
    int64_t *cptr, *cnp, *choff[2];
    uint32_t *key[2], *skey[2];
    int32_t *val, *perm[2], *lo[2], *hi[2], *kept, *nch[2];
    double *dis, *lw;
    void* scan_tmp; size_t scan_bytes;
    void* sort_tmp; size_t sort_bytes;
};

size_t carve_build(Carve& C, int64_t m, int64_t S, int64_t G, int64_t N, int flags, Bufs& B) {
    const int64_t slots = (S / G) * N;
    B.err = C.take<int32_t>(GCN_ERR_WORDS);
    B.cnt = C.take<unsigned long long>(CNT_WORDS);
    B.cptr = C.take<int64_t>(S + 1);
    B.cnp = C.take<int64_t>(G + 1);
    B.val = C.take<int32_t>(m);
    B.dis = C.take<double>(slots);
    B.lw = C.take<double>(slots);
    B.kept = C.take<int32_t>(slots + 1);
    for (int d = 0; d < 2; ++d) {
        const bool has = d == 0 || (flags & RLAP_PLAN_TRANSPOSED) != 0;   // (the sort by target serves the degrees of every build)
        B.key[d] = C.take<uint32_t>(m);   // (the key pass writes both)
        B.skey[d] = C.take<uint32_t>(has ? m : 0);
        B.perm[d] = C.take<int32_t>(has ? m : 0);
        B.lo[d] = C.take<int32_t>(has ? slots : 0);
        B.hi[d] = C.take<int32_t>(has ? slots : 0);
        B.nch[d] = C.take<int32_t>(slots + 1);
        B.choff[d] = C.take<int64_t>(slots + 1);
    }
    B.scan_bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, B.scan_bytes, (const int32_t*)nullptr, (int64_t*)nullptr, (int64_t)0, (size_t)(slots + 1),
                                  rocprim::plus<int64_t>(), (hipStream_t)0);
    B.scan_tmp = C.take<char>((int64_t)B.scan_bytes);
    B.sort_bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, B.sort_bytes, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const int32_t*)nullptr,
                                    (int32_t*)nullptr, (size_t)std::max<int64_t>(m, 1), 0u, edgeplan::key_bits(slots), (hipStream_t)0);
    B.sort_tmp = C.take<char>((int64_t)B.sort_bytes);
    return C.off + 256;
}

}  // namespace

size_t edge_plan_build_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int flags) {
    Carve C{nullptr, 0};
    Bufs B;
    return carve_build(C, m, S, G, N, flags, B);
}

int edge_plan_build_run(hipStream_t st, void* ws, size_t ws_bytes, const SnapshotPlanArgs& g, rlap_plan_desc* desc, SnapshotPlanReport* rep) {
    *rep = SnapshotPlanReport{};
    const SnapshotSeg& in = g.seg;
    const int64_t m = in.m, S = in.S, G = in.G, N = in.N, slots = (S / G) * N;
    if (slots >= edgeplan::MAX_SLOTS) return RLAP_E_TOO_LARGE;
    Bufs B;
    Carve C{static_cast<char*>(ws), 0};
    if (carve_build(C, m, S, G, N, g.flags, B) > ws_bytes) return RLAP_E_WORKSPACE;
    const bool want[2] = {(g.flags & RLAP_PLAN_FORWARD) != 0, (g.flags & RLAP_PLAN_TRANSPOSED) != 0};
    const int loops = (g.flags & RLAP_GCN_SELF_LOOPS) ? 1 : 0, normalize = (g.flags & RLAP_GCN_NORMALIZE) ? 1 : 0;
    const int weighted = (g.flags & RLAP_GCN_WEIGHTED) ? 1 : 0;
    const plan::Layout L = plan::layout(m, slots, loops != 0, want[0], want[1]);
    if ((size_t)L.bytes > g.plan_bytes) return RLAP_E_BAD_ARG;
    char* pb = static_cast<char*>(g.plan);
    Eb a{};
    a.sc = in.sc; a.m = m; a.ptr = B.cptr; a.S = S; a.node_ptr = in.node_ptr ? B.cnp : nullptr; a.G = G; a.N = N; a.slots = slots;
    a.weighted = weighted; a.loops = loops; a.normalize = normalize; a.fill = g.fill;
    for (int d = 0; d < 2; ++d) { a.key[d] = B.key[d]; a.skey[d] = B.skey[d]; a.perm[d] = B.perm[d]; a.lo[d] = B.lo[d]; a.hi[d] = B.hi[d]; }
    a.dis = B.dis; a.lw = B.lw; a.cnt = B.cnt; a.err = B.err;
    a.kept = B.kept; a.dcap = plan::dir_cap(m);
    // 1. the tables, checked and copied; the keys; the sorts and the range of every slot
    RLAP_HIPCHK(hipMemsetAsync(B.err, 0, sizeof(int32_t) * GCN_ERR_WORDS, st));
    RLAP_HIPCHK(hipMemsetAsync(B.cnt, 0, sizeof(unsigned long long) * CNT_WORDS, st));
    const int rc = gcn_tables_enqueue(st, in.ptr, S, m, in.node_ptr, G, N, B.cptr, B.cnp, B.err);
    if (rc != RLAP_OK) return rc;
    const bool sorted[2] = {true, want[1]};
    for (int d = 0; d < 2; ++d) {
        if (!sorted[d] || slots == 0) continue;
        RLAP_HIPCHK(hipMemsetAsync(B.lo[d], 0, sizeof(int32_t) * (size_t)slots, st));
        RLAP_HIPCHK(hipMemsetAsync(B.hi[d], 0, sizeof(int32_t) * (size_t)slots, st));
    }
    if (m > 0) {
        const int vec = (reinterpret_cast<uintptr_t>(in.sc) & 15) == 0 ? 1 : 0;
        hipLaunchKernelGGL(k_ep_keys, dim3(ep_blocks((m + 1) / 2, EP_THREADS)), dim3(EP_THREADS), 0, st, a, vec, weighted && normalize, B.val);
        RLAP_HIPCHK(hipGetLastError());
        for (int d = 0; d < 2; ++d) {
            if (!sorted[d]) continue;
            size_t sb = B.sort_bytes;
            RLAP_HIPCHK(rocprim::radix_sort_pairs(B.sort_tmp, sb, (const uint32_t*)B.key[d], B.skey[d], (const int32_t*)B.val, B.perm[d], (size_t)m,
                                                0u, edgeplan::key_bits(slots), st));
            hipLaunchKernelGGL(k_ep_bounds, dim3(ep_blocks(m, EP_THREADS)), dim3(EP_THREADS), 0, st, a, d);
            RLAP_HIPCHK(hipGetLastError());
        }
    }
    // 2. the degrees of every slot
    if (slots > 0 && (normalize || loops)) {
        hipLaunchKernelGGL(k_ep_degree, dim3(ep_blocks(slots * edgeplan::LANES, EP_THREADS)), dim3(EP_THREADS), 0, st, a);
        RLAP_HIPCHK(hipGetLastError());
    }
    // 3. per direction: counts, scans, records, directory
    bool loop_written = false;
    for (int d = 0; d < 2; ++d) {
        if (!want[d]) continue;
        a.transpose = d;
        a.nch = B.nch[d]; a.choff = B.choff[d];
        a.off = reinterpret_cast<int64_t*>(pb + L.off[d]);
        a.rec = reinterpret_cast<plan::Record*>(pb + L.rec[d]);
        a.dir = reinterpret_cast<plan::ChunkRef*>(pb + L.dir[d]);
        a.loopc = (loops && !loop_written) ? reinterpret_cast<double*>(pb + L.loop) : nullptr;
        loop_written = true;
        hipLaunchKernelGGL(k_ep_count, dim3(ep_blocks(slots + 1, EP_THREADS)), dim3(EP_THREADS), 0, st, a);
        RLAP_HIPCHK(hipGetLastError());
        size_t cb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.kept, a.off, (int64_t)0, (size_t)(slots + 1), rocprim::plus<int64_t>(), st));
        cb = B.scan_bytes;
        RLAP_HIPCHK(rocprim::exclusive_scan(B.scan_tmp, cb, B.nch[d], B.choff[d], (int64_t)0, (size_t)(slots + 1), rocprim::plus<int64_t>(), st));
        if (m > 0) {
            hipLaunchKernelGGL(k_ep_fill, dim3(ep_blocks(m, EP_THREADS)), dim3(EP_THREADS), 0, st, a);
            if (loops) hipLaunchKernelGGL(k_ep_fill_walk, dim3(ep_blocks(slots, EP_THREADS)), dim3(EP_THREADS), 0, st, a);
            if (a.dcap > 0) hipLaunchKernelGGL(k_ep_dir, dim3(ep_blocks(slots, EP_THREADS)), dim3(EP_THREADS), 0, st, a);
            RLAP_HIPCHK(hipGetLastError());
        }
    }
    // 4. the error words, the counts and the last scan entries, read back once
    int32_t herr[GCN_ERR_WORDS];
    unsigned long long hcnt[CNT_WORDS];
    int64_t hent[2] = {0, 0}, hch[2] = {0, 0};
    RLAP_HIPCHK(hipMemcpyAsync(herr, B.err, sizeof(herr), hipMemcpyDeviceToHost, st));
    RLAP_HIPCHK(hipMemcpyAsync(hcnt, B.cnt, sizeof(hcnt), hipMemcpyDeviceToHost, st));
    for (int d = 0; d < 2; ++d) {
        if (!want[d]) continue;
        RLAP_HIPCHK(hipMemcpyAsync(&hent[d], reinterpret_cast<int64_t*>(pb + L.off[d]) + slots, 8, hipMemcpyDeviceToHost, st));
        RLAP_HIPCHK(hipMemcpyAsync(&hch[d], B.choff[d] + slots, 8, hipMemcpyDeviceToHost, st));
    }
    RLAP_HIPCHK(hipStreamSynchronize(st));
    rep->host_syncs = 1;
    if (herr[GCN_ERR_ARG]) return RLAP_E_BAD_ARG;
    if (herr[COL_ERR_RANGE]) return RLAP_E_INDEX_RANGE;
    if (herr[GCN_ERR_WEIGHT]) return RLAP_E_BAD_ARG;
    const int64_t removed = loops ? (int64_t)hcnt[CNT_LOOPS] : 0;
    rep->loops_removed = removed;
    rep->entries = m + (loops ? slots - removed : 0);
    rep->blocks = (int64_t)hcnt[CNT_BLOCKS];
    int64_t used = 256;
    for (int d = 0; d < 2; ++d) {
        rep->dir_entries[d] = want[d] ? hent[d] : -1;
        rep->dir_chunks[d] = want[d] ? hch[d] : -1;
        rep->chunked[d] = want[d] ? (int64_t)hcnt[d ? CNT_CHUNKED_T : CNT_CHUNKED_F] : -1;
        if (!want[d]) continue;
        if (hent[d] < 0 || hent[d] > m || hch[d] < 0 || hch[d] > a.dcap) return RLAP_E_INTERNAL;
        used = std::max<int64_t>(used, L.rec[d] + (int64_t)sizeof(plan::Record) * hent[d]);
        used = std::max<int64_t>(used, L.dir[d] + (int64_t)sizeof(plan::ChunkRef) * a.dcap);
    }
    *desc = rlap_plan_desc{};
    desc->m = m; desc->segments = S; desc->graphs = G; desc->num_nodes = N; desc->fill_value = g.fill;
    desc->entries_forward = rep->dir_entries[0]; desc->entries_transposed = rep->dir_entries[1];
    desc->chunks_forward = rep->dir_chunks[0]; desc->chunks_transposed = rep->dir_chunks[1];
    desc->loop_offset = L.loop;
    desc->off_forward = L.off[0]; desc->dir_forward = L.dir[0]; desc->rec_forward = L.rec[0];
    desc->off_transposed = L.off[1]; desc->dir_transposed = L.dir[1]; desc->rec_transposed = L.rec[1];
    desc->plan_bytes = plan::align_up(used);
    desc->flags = g.flags;
    desc->magic = plan::MAGIC;
    return RLAP_OK;
}

}  // namespace rlap
