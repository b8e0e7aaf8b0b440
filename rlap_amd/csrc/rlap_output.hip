// rlap_output.hip -- the output pass of a call, behind the round kernels (rlap_kernels.hip).
//
//   K9  k_sc_keys/k_sc_ext/k_sc_tierlists/k_sc_merge_half/k_sc_merge_t<cap>/k_sc_merge_big/k_sc_merge_mw<waves>/k_sc_merge_huge/
//       k_sc_compact/k_graph_rows   output (preconditioner.cc:435-457,312-345)
//   block_std_sort           libstdc++ std::sort's permutation of one array by several waves (the others: rlap_wave_sort.h)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rlap_core.h"
#include "rlap_kernels.h"
#include "rlap_wave_sort.h"

namespace rlap {

// ---------------------------------------------------------------------------
// K9: output.  sc_keys/sc_perm: pop order of the surviving vertices;
// sc_merge (pass A): per vertex gather -> sort -> merge -> order -> staging;
// sc_compact (pass B): prefix-sum compaction of the staged rows into (m,3) f64.
// ---------------------------------------------------------------------------
__global__ void k_sc_keys(const VRec* __restrict__ vr, const int32_t* __restrict__ origpos,
                          const int32_t* __restrict__ vgraph, const GraphDesc* __restrict__ gd, int32_t N,
                          uint64_t* __restrict__ skey, uint32_t* __restrict__ sval) {
    int32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    const VRec me = vr[v];
    int32_t pp = me.pqpos;
    uint64_t k = ~0ull;
    if (pp != -2) {
        const GraphDesc& D = gd[vgraph[v]];
        uint32_t b = (uint32_t)(D.bucket_base + pq_list_of(me.key, D.n));
        uint32_t ord = pp >= 0 ? (0x7FFFFFFFu - (uint32_t)pp) : (0x80000000u + (uint32_t)origpos[v]);
        k = ((uint64_t)b << 32) | ord;
    }
    skey[v] = k;
    sval[v] = (uint32_t)v;
}

__global__ void k_sc_perm_order(const int64_t* __restrict__ perm, const int32_t* __restrict__ vgraph, const GraphDesc* __restrict__ gd,
                                const int64_t* __restrict__ surv_base, int32_t N, uint32_t* __restrict__ order) {
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int32_t g = vgraph[i];
    const GraphDesc& D = gd[g];
    int32_t idx = i - D.vbase;              // position in the node_id vector
    int64_t q = (int64_t)D.n - 1 - idx;     // pop number (0-based)
    int64_t pl = perm[i];
    if (pl < 0 || pl >= (int64_t)D.n) pl = 0;   // invalid entry (flagged by k_perm_check; the call fails): keep the index in range
    if (q >= D.n_elim) order[surv_base[g] + (q - D.n_elim)] = (uint32_t)(D.vbase + (int32_t)pl);
}

// Rejected input (range / cross-graph / node_id flags, asymmetry: the same tests the elimination kernel makes) gives every column
// the extent 0: the output pass then stages and writes nothing -- an invalid node_id vector can name one hub S times, which would
// run past the staging arrays (sized one row per slot in use).
__global__ void k_sc_ext(const uint32_t* __restrict__ order, const int32_t* __restrict__ colptr, const VRec* __restrict__ vr,
                         int32_t S, const int32_t* __restrict__ in_flags, const double* __restrict__ in_acc, int32_t* __restrict__ ext,
                         const int32_t* __restrict__ stop) {
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S) return;
    // (stop: a depths call's status word -- after a failed segment the later snapshots stage nothing either)
    const bool bad = in_flags[FLAG_RANGE] || in_flags[FLAG_CROSS] || in_flags[FLAG_PERM] || in_acc[2] != 0.0 || !(in_acc[0] <= 1e-24 * in_acc[1]) ||
                     (stop && *stop != 0);
    int32_t v = (int32_t)order[i];
    ext[i] = bad ? 0 : (colptr[v + 1] - colptr[v]) + vr[v].app_cnt;
}

// where a workgroup of the merge kernels adds the live entries it saw: one of LIVE_SLOTS counters, LIVE_STRIDE words apart
__device__ __forceinline__ unsigned long long* live_slot(unsigned long long* live_total) { return &live_total[(blockIdx.x & (LIVE_SLOTS - 1)) * LIVE_STRIDE]; }

template <int CAP>
struct ScLdsT {
    SRec rec[CAP];
    double a_val[CAP];
    double b_val[CAP];
    int32_t a_nbr[CAP];
    int32_t b_nbr[CAP];
    int32_t rank[CAP];
};

template <bool GREATER, class LDS, class KeyF>
__device__ __forceinline__ bool sc_rank_sort(LDS& L, int cnt, KeyF keyf, int lane) {
    bool dup = false;
    for (int i = lane; i < cnt; i += 64) {
        double ki = keyf(i);
        int rank = 0;
        for (int j = 0; j < cnt; ++j) {
            double kj = keyf(j);
            bool before = GREATER ? (kj > ki) : (kj < ki);
            bool eq = (kj == ki);
            rank += (before || (eq && j < i)) ? 1 : 0;
            dup |= (eq && j != i);
        }
        L.rank[i] = rank;
    }
    bool anydup = __ballot(dup) != 0ull;
    if (cnt > 16 && anydup) return false;
    for (int i = lane; i < cnt; i += 64) {
        int r = L.rank[i];
        L.rec[r].key = keyf(i);
        L.rec[r].idx = i;
    }
    return true;
}

// CAP = LDS capacity per column; columns with extent in (LO, CAP] are taken, the others left to the other
// instantiation / the long-column kernel.  The small instantiation (CAP 64) keeps ~30 waves per CU resident.
template <int CAP, int LO>
__global__ __launch_bounds__(64) void k_sc_merge_t(Arrays A, const GraphDesc* __restrict__ gd, const int32_t* __restrict__ vgraph,
                                                   const uint32_t* __restrict__ order, const int32_t* __restrict__ ext,
                                                   const int64_t* __restrict__ tmp_off, int32_t S, int32_t* __restrict__ tmp_nbr,
                                                   double* __restrict__ tmp_val, int32_t* __restrict__ cnt_out, ScScratch SS,
                                                   unsigned long long* __restrict__ live_total, const int32_t* __restrict__ worklist,
                                                   const int32_t* __restrict__ workcount) {
    __shared__ ScLdsT<CAP> L;
    __shared__ WaveSortScratchT<CAP> WS;
    __shared__ int32_t s_tmp64[CAP == 64 ? 144 : 1];
    const WaveSortPtrs WP = {WS.ulist, WS.dlist, WS.segmark, WS.stk};
    const int lane = lane_id();
    const uint64_t lt = lanemask_lt(lane);
    (void)S;
    // columns of at most 64 entries: std::sort's permutation with one element per lane (registers + shuffles);
    // leaves L.rec[position] = {key, source index} like the LDS paths.  False: depth limit hit, use those.
    auto sort64 = [&](const double keyv, const int cnt, const bool greater) -> bool {
        if (CAP != 64) return false;
        double key = keyv;
        int idx = lane, pos = lane;
        const bool ok = greater ? wave_sort64<true>(key, idx, cnt, lane, s_tmp64, &pos) : wave_sort64<false>(key, idx, cnt, lane, s_tmp64, &pos);
        if (ok && lane < cnt) { L.rec[pos].key = key; L.rec[pos].idx = idx; }
        __syncthreads();
        return ok;
    };
    constexpr int RT = (CAP + 63) / 64;
    constexpr bool RANK_FIRST = CAP <= 64;   // longer columns: the stable rank is O(n^2/64), the restatement O(n log n / 64)
    // L.rec[position] = {key, source index} of cnt entries in std::sort's order of keyf(source index), descending if `greater` (a
    // std::true_type or std::false_type): sort64, then the stable rank where it is exact, then the restatement in LDS
    auto order_by = [&](const int cnt, auto keyf, auto greater) {
        constexpr bool GT = decltype(greater)::value;
        using Less = std::conditional_t<GT, SRecGreaterKey, SRecLessKey>;
        if (sort64(lane < cnt ? keyf(lane) : 0.0, cnt, GT)) return;
        const bool done = RANK_FIRST ? sc_rank_sort<GT>(L, cnt, keyf, lane) : false;
        __syncthreads();
        if (done) return;
        for (int q = lane; q < cnt; q += 64) { L.rec[q].key = keyf(q); L.rec[q].idx = q; }
        __syncthreads();
        wave_std_sort<SRec, Less, RT>(L.rec, cnt, Less(), WP, lane);
        __syncthreads();
    };
    const int32_t nwork = *workcount;
    unsigned long long live_acc = 0ull;   // lane 0: live entries seen by this workgroup (one atomic at the end, spread over LIVE_SLOTS counters)
    for (int32_t wi = blockIdx.x; wi < nwork; wi += gridDim.x) {
        const int32_t i = worklist[wi];   // lists are filled with atomics: heavy columns end up spread over the grid
        const int32_t v = (int32_t)order[i];
        const int64_t toff = tmp_off[i];
        const int32_t ex = ext[i];
        if (CAP == SCAP && ex > SCAP) {   // (only the last tier's list can hold such a column: the other instantiations stay lean)
            // long column: k_sc_merge_big / k_sc_merge_huge take it, unless it is too long even for their 16-bit stop lists:
            // then the sequential form in global scratch (one lane)
            if (lane == 0 && ex > HUGECAP) {
                unsigned long long off = atomicAdd(SS.top, (unsigned long long)ex);
                if ((int64_t)(off + (unsigned long long)ex) > SS.cap) { SS.flags[FLAG_SCR] = 1; cnt_out[i] = 0; }   // scratch budget too small: the call is repeated with more
                else {
                ColBuf B = SS.colbuf((int64_t)off);
                GraphDesc D = gd[vgraph[v]];
                int32_t len0 = serial_gather(A, v, B, ex);
                int32_t m = serial_sort_merge(A, D, B, len0, false, false);
                Arrays Ag = A;
                Ag.shuffle_seed = A.shuffle_seed + (uint64_t)vgraph[v];
                serial_order(Ag, B, m, v, 1, D.vbase);
                for (int j = 0; j < m; ++j) { tmp_nbr[toff + j] = B.a_nbr[j]; tmp_val[toff + j] = B.a_val[j]; }
                cnt_out[i] = m;
                live_acc += (unsigned long long)len0;
                }
            }
            __syncthreads();
            continue;
        }
        const int len0 = wave_col_live(A, v, lane, [&](int pos, int32_t, const Slot& g) { L.a_nbr[pos] = g.nbr; L.a_val[pos] = g.val; });
        __syncthreads();
        order_by(len0, [&](int q) { return (double)L.a_nbr[q]; }, std::false_type());   // by id (:314-315)
        // merge (:317-329): head = first of its id group; sums in sorted order
        int m = 0;
        {
            int carry = 0;
            for (int i0 = 0; i0 < len0; i0 += 64) {
                int q = i0 + lane;
                bool act = q < len0;
                int32_t nb = act ? L.a_nbr[L.rec[q].idx] : -1;
                int32_t nbprev = (q > 0 && act) ? L.a_nbr[L.rec[q - 1].idx] : -2;
                bool head = act && nb != nbprev;
                uint64_t mask = __ballot(head);
                int x = carry + popc64(mask & lt);
                if (head) {
                    double val = L.a_val[L.rec[q].idx];
                    for (int z = q + 1; z < len0 && L.a_nbr[L.rec[z].idx] == nb; ++z) val += L.a_val[L.rec[z].idx];
                    L.b_nbr[x] = nb; L.b_val[x] = val;
                }
                carry += popc64(mask);
            }
            m = carry;
        }
        __syncthreads();
        // order by o_n (:331-343)
        if (keyed_order(A)) {
            const int32_t gi = vgraph[v], vb = gd[gi].vbase;
            const uint64_t kb = keyed_order_base(A.shuffle_seed + (uint64_t)gi, v - vb, 1);
            order_by(m, [&](int q) { return keyed_order_dkey(kb, L.b_nbr[q] - vb); }, std::false_type());
        } else if (A.o_n == ON_ASC) order_by(m, [&](int q) { return L.b_val[q]; }, std::false_type());
        else order_by(m, [&](int q) { return L.b_val[q]; }, std::true_type());
        for (int j = lane; j < m; j += 64) {
            int x = L.rec[j].idx;
            tmp_nbr[toff + j] = L.b_nbr[x];
            tmp_val[toff + j] = L.b_val[x];
        }
        if (lane == 0) { cnt_out[i] = m; live_acc += (unsigned long long)len0; }
        __syncthreads();
    }
    if (lane == 0 && live_acc) atomicAdd(live_slot(live_total), live_acc);
}

// work lists per capacity tier (5: <=32 (two columns per wave), 0: <=64, 1: <=192, 2: <=512 and what the long-column kernels
// do not take, 3: k_sc_merge_big, 4: k_sc_merge_huge)
__global__ __launch_bounds__(1024) void k_sc_tierlists(const int32_t* __restrict__ ext, int32_t S, int32_t keyed, int32_t* __restrict__ lists, int32_t* __restrict__ counts) {
    __shared__ int32_t s_cnt[8], s_base[8];
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int tier = -1;
    (void)keyed;
    if (threadIdx.x < 8) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if (i < S) {
        int32_t e = ext[i];
        tier = e <= 32 ? 5 : e <= 64 ? 0 : (e <= 192 ? 1 : ((e > SCAP && e <= HUGECAP) ? (e <= MID1CAP ? 7 : (e <= MIDCAP ? 6 : (e <= BIGCAP ? 3 : 4))) : 2));
    }
    // one LDS atomic per wave and tier, one global atomic per workgroup and tier (same-address atomics serialise):
    // neighbouring columns stay neighbours in the list (locality of the staged rows)
    int32_t my = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        uint64_t mk = __ballot(tier == t);
        if (mk == 0ull) continue;
        int32_t base = 0;
        const int leader = __builtin_ctzll(mk);
        if (lane == leader) base = atomicAdd(&s_cnt[t], __popcll(mk));
        base = __shfl(base, leader);
        if (tier == t) my = base + __popcll(mk & lanemask_lt(lane));
    }
    __syncthreads();
    if (threadIdx.x < 8 && s_cnt[threadIdx.x] > 0) s_base[threadIdx.x] = atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
    __syncthreads();
    if (tier >= 0) lists[(size_t)tier * S + s_base[tier] + my] = i;
}

// Columns of at most 32 slots (most of them after half the vertices are gone): TWO per wave, one per half-wave, entirely
// in registers -- the column is read one slot per lane, compacted, ordered by id and by o_n with group_sort<32> (the
// std::sort restatement for two 32-lane groups), merged with shuffles, and stored from the lanes.  A column whose sort
// hits the depth limit is handed to the 64-entry kernel's list.
__global__ __launch_bounds__(64) void k_sc_merge_half(Arrays A, const GraphDesc* __restrict__ gd, const int32_t* __restrict__ vgraph,
                                                      const uint32_t* __restrict__ order, const int64_t* __restrict__ tmp_off,
                                                      int32_t* __restrict__ tmp_nbr, double* __restrict__ tmp_val, int32_t* __restrict__ cnt_out,
                                                      unsigned long long* __restrict__ live_total, const int32_t* __restrict__ worklist,
                                                      const int32_t* __restrict__ workcount, int32_t* __restrict__ list64, int32_t* __restrict__ count64) {
    __shared__ int32_t s_tmp[2 * (2 * 34 + 12)];
    const int lane = lane_id();
    const int gl = lane & 31, gbase = lane & 32;
    const uint64_t gmask = 0xFFFFFFFFull << gbase;
    const uint64_t lt = lanemask_lt(lane) & gmask;
    const bool keyed = keyed_order(A);
    const bool desc = (A.o_n == ON_DESC) && !keyed;
    const int32_t nwork = *workcount;
    unsigned long long live_acc = 0ull;   // lanes 0 and 32
    auto to_lane = [&](int target, int v) { return __builtin_amdgcn_ds_permute((gbase + target) << 2, v); };   // forward permute inside the half
    auto to_lane_d = [&](int target, double v) {
        const long long b = __double_as_longlong(v);
        const int lo = to_lane(target, (int)(uint32_t)b), hi = to_lane(target, (int)(uint32_t)((unsigned long long)b >> 32));
        return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
    };
    for (int32_t w0 = 2 * blockIdx.x; w0 < nwork; w0 += 2 * gridDim.x) {
        const int32_t wi = w0 + (lane >> 5);
        const bool have = wi < nwork;
        int32_t i = 0, v = 0, cp1 = 0, acnt = 0, ext = 0, cb0 = 0, cb1 = 0, cb2 = 0;
        int64_t toff = 0;
        if (have) {
            i = worklist[wi];
            v = (int32_t)order[i];
            toff = tmp_off[i];
            const int32_t cp0 = A.colptr[v];
            cp1 = A.colptr[v + 1];
            acnt = A.vr[v].app_cnt;
            ext = (cp1 - cp0) + acnt;
            if (acnt > 0) {   // bases of the (at most three) appended chunks
                const int ct = chunk_of(acnt - 1);
                int32_t base = A.vr[v].app_chunk;
                if (ct == 2) { cb2 = base; base = A.e[base].nbr; }
                if (ct >= 1) { cb1 = base; base = A.e[base].nbr; }
                cb0 = base;
            }
        }
        // one slot per lane, in the traversal order of :248-271 (appended entries newest first, then the CSR segment backwards)
        double val = 0; int32_t nb = 0;
        if (gl < ext) {
            int32_t sl;
            if (gl < acnt) { const int32_t a = acnt - 1 - gl; const int c = chunk_of(a); sl = (c == 0 ? cb0 : c == 1 ? cb1 : cb2) + 1 + (a - chunk_start(c)); }
            else sl = cp1 - 1 - (gl - acnt);
            val = A.e[sl].val; nb = A.e[sl].nbr;
        }
        const bool live = gl < ext && val > 0;
        const uint64_t lm = __ballot(live) & gmask;
        const int nlive = __popcll(lm);
        // compact the live entries to the front of the half (a permutation: dead lanes go behind)
        {
            const int below = __popcll(lm & lt);
            const int target = live ? below : nlive + (gl - below);
            nb = to_lane(target, nb);
            val = to_lane_d(target, val);
        }
        // order by id (:314-315)
        bool ok = true;
        {
            double key = (double)nb; int idx = gl, pos = gl;
            const bool want = have && nlive > 1;
            const bool okg = group_sort<false, 32>(key, idx, nlive, want, lane, s_tmp, &pos);
            if (want) {
                ok = okg;
                const double ve = __shfl(val, gbase + idx);
                const int target = gl < nlive ? pos : gl;
                nb = to_lane(target, (int32_t)key);
                val = to_lane_d(target, ve);
            }
        }
        // merge (:317-329): the first of a run of equal ids takes the sum, in sorted order
        int m = nlive;
        {
            const int32_t nbp = __shfl_up(nb, 1);
            const bool head = gl < nlive && (gl == 0 || nb != nbp);
            const uint64_t hm = __ballot(head) & gmask;
            m = __popcll(hm);
            if (m != nlive) {   // (group-uniform)
                double acc = val;
                const uint64_t above = (gl == 31) ? 0ull : ((hm >> (lane + 1)) & (0xFFFFFFFFull >> (gl + 1)));
                const int nexthead = above ? (gl + 1 + __builtin_ctzll(above)) : nlive;
                for (int q = 1; q < 32; ++q) {   // shuffles must be executed by the whole half: fixed trip count, predicated adds
                    const double vq = __shfl(val, gbase + ((gl + q) & 31));
                    if (head && gl + q < nexthead) acc += vq;
                }
                const int below = __popcll(hm & lt);
                const int target = head ? below : (gl < nlive ? m + (gl - below) : gl);
                nb = to_lane(target, nb);
                val = to_lane_d(target, acc);
            }
        }
        // order by o_n (:331-343) and store from the lanes
        {
            double key = val;
            if (keyed && have) {
                const int32_t gi = vgraph[v], vb = gd[gi].vbase;
                key = keyed_order_dkey(keyed_order_base(A.shuffle_seed + (uint64_t)gi, v - vb, 1), nb - vb);
            }
            int idx = gl, pos = gl;
            const bool want = have && m > 1;
            const bool okg = desc ? group_sort<true, 32>(key, idx, m, want, lane, s_tmp, &pos) : group_sort<false, 32>(key, idx, m, want, lane, s_tmp, &pos);
            if (want) ok = ok && okg;
            const int32_t nbo = __shfl(nb, gbase + idx);
            const double vo = __shfl(val, gbase + idx);
            if (have && ok && gl < m) { tmp_nbr[toff + pos] = nbo; tmp_val[toff + pos] = vo; }
        }
        if (have && gl == 0) {
            if (ok) { cnt_out[i] = m; live_acc += (unsigned long long)nlive; }
            else list64[atomicAdd(count64, 1)] = i;   // depth limit hit: the 64-entry kernel (launched after this one) takes it
        }
    }
    live_acc += __shfl_down(live_acc, 32);
    if (lane == 0 && live_acc) atomicAdd(live_slot(live_total), live_acc);
}

void launch_sc_merge(const ScLaunch& X, const Arrays& A, const GraphDesc* gd, const int32_t* vgraph, const uint32_t* order, const int32_t* ext,
                     const int64_t* tmp_off, int32_t S, int32_t* tmp_nbr, double* tmp_val, int32_t* cnt_out, const ScScratch& SS,
                     unsigned long long* live_total, int32_t* lists, int32_t* counts, uint16_t* hugelists) {
    const int keyed = keyed_order(A) ? 1 : 0;
    hipStream_t stream = X.main;
    hipLaunchKernelGGL(k_sc_tierlists, dim3((S + 1023) / 1024), dim3(1024), 0, stream, ext, S, keyed, lists, counts);
    // the tiers are independent of each other (only the <=64 kernel follows the <=32 one, which hands it the columns whose sort
    // hit the depth limit): the long-column kernels and the LDS tiers run beside the two big tiers on side streams
    const bool fork = X.side[0] && X.side[1];
    hipStream_t s1 = fork ? X.side[0] : stream, s2 = fork ? X.side[1] : stream;
    if (fork) {
        (void)hipEventRecord(X.ev[0], stream);
        (void)hipStreamWaitEvent(s1, X.ev[0], 0);
        (void)hipStreamWaitEvent(s2, X.ev[0], 0);
    }
    // long columns: whole column in LDS, one single-wave workgroup each; longer than the LDS record array (hubs of
    // weighted graphs): records in global scratch, a few workgroups
    // (one workgroup of 8 waves per CU at ~156 KB of LDS: the few columns beyond MIDCAP slots; the tier below: 4 waves, three to a CU)
    // (the <=512 tier goes first on the first side stream: the 8-wave kernel behind it needs a whole CU's LDS per workgroup and waits for
    // one to drain anyway -- config 5 has no such column and the kernel sat there for 4.7 ms; on the main stream this tier was the end of
    // the longest chain, <=32 -> <=64 -> <=512: 4.8 ms)
    unsigned g2 = (unsigned)(S < 256 * 6 * 16 ? S : 256 * 6 * 16);
    hipLaunchKernelGGL((k_sc_merge_t<SCAP, 192>), dim3(g2), dim3(64), 0, s1, A, gd, vgraph, order, ext, tmp_off, S, tmp_nbr, tmp_val, cnt_out, SS, live_total, lists + 2 * (size_t)S, counts + 2);
    hipLaunchKernelGGL((k_sc_merge_mw<8>), dim3(512), dim3(512), MW_BIG_LDS_BYTES, s1, A, gd, vgraph, order, ext, tmp_off, lists + 3 * (size_t)S, counts + 3,
                       tmp_nbr, tmp_val, cnt_out, live_total, (int32_t)BIGCAP, (int32_t)MW_BIG_QCAP);
    hipLaunchKernelGGL((k_sc_merge_mw<4>), dim3(1024), dim3(256), MW_MID_LDS_BYTES, s2, A, gd, vgraph, order, ext, tmp_off, lists + 6 * (size_t)S, counts + 6,
                       tmp_nbr, tmp_val, cnt_out, live_total, (int32_t)MIDCAP, (int32_t)MW_MID_QCAP);
    hipLaunchKernelGGL(k_sc_merge_big, dim3(2048), dim3(64), MID1_LDS_BYTES, s2, A, gd, vgraph, order, ext, tmp_off, lists + 7 * (size_t)S, counts + 7,
                       tmp_nbr, tmp_val, cnt_out, live_total, nullptr, (int32_t)MID1CAP);   // (stop lists in LDS: no global list region)
    hipLaunchKernelGGL(k_sc_merge_huge, dim3(NHUGE), dim3(64), 0, s1, A, gd, vgraph, order, ext, tmp_off, lists + 4 * (size_t)S, counts + 4,
                       tmp_nbr, tmp_val, cnt_out, live_total, hugelists, SS.rec, SS.top, SS.cap, SS.flags);
    unsigned g1 = (unsigned)(S < 256 * 16 * 8 ? S : 256 * 16 * 8);
    hipLaunchKernelGGL((k_sc_merge_t<192, 64>), dim3(g1), dim3(64), 0, s2, A, gd, vgraph, order, ext, tmp_off, S, tmp_nbr, tmp_val, cnt_out, SS, live_total, lists + (size_t)S, counts + 1);
    unsigned gh = (unsigned)(S < 256 * 32 * 4 ? (S + 1) / 2 : 256 * 32 * 4);
    if (gh == 0) gh = 1;
    hipLaunchKernelGGL(k_sc_merge_half, dim3(gh), dim3(64), 0, stream, A, gd, vgraph, order, tmp_off, tmp_nbr, tmp_val, cnt_out, live_total, lists + 5 * (size_t)S, counts + 5, lists, counts);
    unsigned g0 = (unsigned)(S < 256 * 32 * 4 ? S : 256 * 32 * 4);
    hipLaunchKernelGGL((k_sc_merge_t<64, -1>), dim3(g0), dim3(64), 0, stream, A, gd, vgraph, order, ext, tmp_off, S, tmp_nbr, tmp_val, cnt_out, SS, live_total, lists, counts);
    if (fork) {
        (void)hipEventRecord(X.ev[1], s1);
        (void)hipEventRecord(X.ev[2], s2);
        (void)hipStreamWaitEvent(stream, X.ev[1], 0);
        (void)hipStreamWaitEvent(stream, X.ev[2], 0);
    }
}

// Long columns (SCAP < extent <= BIGCAP): one single-wave workgroup per column with the whole
// column in LDS as 16-byte records {id as double, weight}; both sorts are the wave-parallel std::sort
// restatement (exact under ties), gather / merge / stores by the wave.
struct Rec2 { double a; double b; };
struct Rec2LessA { __device__ bool operator()(const Rec2& x, const Rec2& y) const { return x.a < y.a; } };
struct Rec2LessB { __device__ bool operator()(const Rec2& x, const Rec2& y) const { return x.b < y.b; } };
struct Rec2GreaterB { __device__ bool operator()(const Rec2& x, const Rec2& y) const { return x.b > y.b; } };
// keyed neighbour order (o_n = random / coarsen): the key is a hash of the neighbour id, recomputed per comparison
struct Rec2LessKeyed {
    uint64_t kb;
    int32_t vbase;
    __device__ bool operator()(const Rec2& x, const Rec2& y) const { return keyed_order_dkey(kb, (int32_t)x.a - vbase) < keyed_order_dkey(kb, (int32_t)y.a - vbase); }
};
// order by o_n: f(the comparator of column v's merged records)
template <class F>
__device__ __forceinline__ void with_rec2_order(const Arrays& A, const GraphDesc* __restrict__ gd, const int32_t* __restrict__ vgraph, int32_t v, F f) {
    if (keyed_order(A)) {   // :339-343
        const int32_t gi = vgraph[v];
        Rec2LessKeyed lk; lk.vbase = gd[gi].vbase; lk.kb = keyed_order_base(A.shuffle_seed + (uint64_t)gi, v - lk.vbase, 1);
        f(lk);
    } else if (A.o_n == ON_ASC) f(Rec2LessB());
    else f(Rec2GreaterB());   // :331-338
}

// HUGE = false: SCAP < extent <= BIGCAP, records in LDS.  HUGE = true: BIGCAP < extent <= HUGECAP (a hub of a
// weighted graph), records in global scratch (L2), both sorts by the wave-parallel restatement.
template <bool HUGE>
__device__ __forceinline__ void sc_merge_long_body(const Arrays& A, const GraphDesc* __restrict__ gd, const int32_t* __restrict__ vgraph,
                                                   const uint32_t* __restrict__ order, const int32_t* __restrict__ ext,
                                                   const int64_t* __restrict__ tmp_off, const int32_t* __restrict__ list,
                                                   const int32_t* __restrict__ count, int32_t* __restrict__ tmp_nbr,
                                                   double* __restrict__ tmp_val, int32_t* __restrict__ cnt_out,
                                                   unsigned long long* __restrict__ live_total, uint16_t* __restrict__ lists,
                                                   Rec2* lds_R, int32_t lds_cap, Rec2* glob_R, unsigned long long* glob_top, int64_t glob_cap, int32_t* glob_flags) {
    constexpr int LCAP = HUGE ? HUGECAP : BIGCAP;
    __shared__ uint32_t s_segmark[LCAP / 32 + 2];
    __shared__ int32_t s_stk[3 * 48];
    __shared__ unsigned long long s_off;
    // HUGE: the sorts partition in global memory only down to segments of STG records, which are sorted through in LDS (wave_std_sort_staged)
    constexpr int STG = HUGE ? 3072 : 1;
    __shared__ Rec2 s_stg[STG];
    __shared__ uint16_t s_stg_ul[STG + 2], s_stg_dl[STG + 2];
    __shared__ uint32_t s_stg_mark[STG / 32 + 2];
    __shared__ uint32_t s_stg_tab[HUGE ? 512 : 1];
    __shared__ uint16_t s_stg_tab2[HUGE ? 512 : 2];
    WaveSortPtrs WL;   // (assigned, not brace-initialised: a constant aggregate of LDS addresses is rejected as a static initialiser)
    WL.ulist = s_stg_ul; WL.dlist = s_stg_dl; WL.segmark = s_stg_mark; WL.stk = s_stk;
    // stop lists of the partition emulation: in LDS behind the records (long columns), in global scratch, one region per
    // workgroup (huge columns)
    uint16_t* const mylists = HUGE ? lists + (size_t)blockIdx.x * 2 * (LCAP + 2) : reinterpret_cast<uint16_t*>(lds_R + lds_cap);
    const WaveSortPtrs WP = {mylists, mylists + ((HUGE ? LCAP : lds_cap) + 2), s_segmark, s_stk};
    const int lane = lane_id();
    const uint64_t lt = lanemask_lt(lane);
    const int32_t nbig = *count;
    unsigned long long live_acc = 0ull;
    for (int32_t bi = blockIdx.x; bi < nbig; bi += gridDim.x) {
        const int32_t i = list[bi];
        const int32_t v = (int32_t)order[i];
        const int64_t toff = tmp_off[i];
        Rec2* R = lds_R;
        if (HUGE) {
            if (lane == 0) {
                s_off = atomicAdd(glob_top, (unsigned long long)ext[i]);
                if ((int64_t)(s_off + (unsigned long long)ext[i]) > glob_cap) { s_off = ~0ull; glob_flags[FLAG_SCR] = 1; cnt_out[i] = 0; }
            }
            __syncthreads();
            if (s_off == ~0ull) { __syncthreads(); continue; }   // scratch budget too small: the call is repeated with more
            R = glob_R + s_off;
        }
        const int len0 = wave_col_live(A, v, lane, [&](int pos, int32_t, const Slot& g) { R[pos].a = (double)g.nbr; R[pos].b = g.val; });
        __syncthreads();
        // sort by id (:314-315), std::sort semantics (the gather order is the traversal order)
        if constexpr (HUGE) wave_std_sort_staged<Rec2, Rec2LessA, 8>(R, len0, Rec2LessA(), WP.ulist, WP.dlist, s_stk, s_stg, STG, WL, s_stg_tab, s_stg_tab2, lane);
        else wave_std_sort<Rec2>(R, len0, Rec2LessA(), WP, lane);
        __syncthreads();
        // merge (:317-329), 64 positions at a time: heads by ballot, sums in sorted order; all reads of a chunk
        // (its look-ahead included) come before its writes, which land at or below the chunk
        int m = 0;
        for (int32_t p0 = 0; p0 < len0; p0 += 64) {
            const int32_t p = p0 + lane;
            const bool act = p < len0;
            Rec2 me = {0.0, 0.0};
            double prev = -1.0;
            if (act) { me = R[p]; if (p > 0) prev = R[p - 1].a; }
            const bool head = act && me.a != prev;
            if (head) for (int32_t q = p + 1; q < len0 && R[q].a == me.a; ++q) me.b += R[q].b;
            const uint64_t mask = __ballot(head);
            const int32_t x = m + popc64(mask & lt);
            __syncthreads();
            if (head) R[x] = me;
            __syncthreads();
            m += popc64(mask);
        }
        with_rec2_order(A, gd, vgraph, v, [&](auto less) {
            if constexpr (HUGE) wave_std_sort_staged<Rec2, decltype(less), 8>(R, m, less, WP.ulist, WP.dlist, s_stk, s_stg, STG, WL, s_stg_tab, s_stg_tab2, lane);
            else wave_std_sort<Rec2>(R, m, less, WP, lane);
        });
        __syncthreads();
        for (int32_t j = lane; j < m; j += 64) { tmp_nbr[toff + j] = (int32_t)R[j].a; tmp_val[toff + j] = R[j].b; }
        if (lane == 0) { cnt_out[i] = m; live_acc += (unsigned long long)len0; }
        __syncthreads();
    }
    if (lane == 0 && live_acc) atomicAdd(live_slot(live_total), live_acc);
}

__global__ __launch_bounds__(64) void k_sc_merge_big(Arrays A, const GraphDesc* __restrict__ gd, const int32_t* __restrict__ vgraph,
                                                     const uint32_t* __restrict__ order, const int32_t* __restrict__ ext,
                                                     const int64_t* __restrict__ tmp_off, const int32_t* __restrict__ list,
                                                     const int32_t* __restrict__ count, int32_t* __restrict__ tmp_nbr,
                                                     double* __restrict__ tmp_val, int32_t* __restrict__ cnt_out,
                                                     unsigned long long* __restrict__ live_total, uint16_t* __restrict__ lists, int32_t lcap) {
    extern __shared__ Rec2 R_lds[];   // lcap records, then the two stop lists of the sort
    sc_merge_long_body<false>(A, gd, vgraph, order, ext, tmp_off, list, count, tmp_nbr, tmp_val, cnt_out, live_total, lists, R_lds, lcap, nullptr, nullptr, 0, nullptr);
}

// ---------------------------------------------------------------------------
// The same restatement of std::sort for ONE array shared by several waves (long surviving columns).  The introsort loop is
// run level by level: every segment longer than 16 that exists at a level is partitioned by one wave (the wave-parallel
// Hoare partition of wave_std_sort, its stop lists kept at the segment's own offsets), its two parts are queued for the next
// level or marked as final; a workgroup barrier separates the levels.  The order in which segments are partitioned does not
// matter (they are disjoint and std::sort's recursion treats them independently), so the permutation is std::sort's.
// The final insertion sort (independent stable sorts of the marked segments) is spread over all threads.
// segq: two queues of QCAP segments (first, last, depth); qcnt[2]; segmark: (n+31)/32+1 words.
// ---------------------------------------------------------------------------
template <class T, class Less, int NW>
__device__ void block_std_sort(T* a, const int n, Less less, uint16_t* ulist, uint16_t* dlist, uint32_t* segmark, int32_t* segq, int32_t* qcnt, const int QCAP) {
    constexpr int NTB = NW * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t lt = lanemask_lt(lane);
    for (int q = tid; q < (n + 31) / 32 + 1; q += NTB) segmark[q] = 0u;
    if (tid == 0) {
        int depth0 = 0;
        for (unsigned q = (unsigned)n; q > 1u; q >>= 1) ++depth0;
        qcnt[0] = n > 16 ? 1 : 0; qcnt[1] = 0;
        segq[0] = 0; segq[1] = n; segq[2] = 2 * depth0;
    }
    __syncthreads();
    if (n < 2) return;
    if (n <= 16) {
        if (tid == 0) gs_insertion_sort<T>(a, n, less);
        __syncthreads();
        return;
    }
    int cur = 0;
    while (true) {
        const int ncur = qcnt[cur];
        if (ncur == 0) break;
        int32_t* const qin = segq + cur * 3 * QCAP;
        int32_t* const qout = segq + (cur ^ 1) * 3 * QCAP;
        for (int sidx = wave; sidx < ncur; sidx += NW) {
            const int first = qin[3 * sidx], last = qin[3 * sidx + 1];
            int depth = qin[3 * sidx + 2];
            if (depth == 0) {   // depth limit: heap sort (std::__partial_sort), by one lane; the segment stays one sorted run
                if (lane == 0) { gs_heap_sort<T>(a, first, last, less); atomicOr(&segmark[first >> 5], 1u << (first & 31)); }
                WAVE_SYNC();
                continue;
            }
            --depth;
            if (lane == 0) {   // __move_median_to_first(first, first+1, mid, last-1)
                int ia = first + 1, ib = first + (last - first) / 2, ic = last - 1;
                int pick;
                if (less(a[ia], a[ib])) {
                    if (less(a[ib], a[ic])) pick = ib;
                    else if (less(a[ia], a[ic])) pick = ic;
                    else pick = ia;
                } else if (less(a[ia], a[ic])) pick = ia;
                else if (less(a[ib], a[ic])) pick = ic;
                else pick = ib;
                T t = a[first]; a[first] = a[pick]; a[pick] = t;
            }
            WAVE_SYNC();
            const T pv = a[first];
            uint16_t* const ul = ulist + first;
            uint16_t* const dl = dlist + first;
            int nu = 0, nd = 0;
            for (int p0 = first + 1; p0 < last; p0 += 64) {
                int p = p0 + lane;
                bool stop = (p < last) && !less(a[p], pv);
                uint64_t mk = __ballot(stop);
                if (stop) ul[nu + popc64(mk & lt)] = (uint16_t)p;
                nu += popc64(mk);
            }
            for (int p0 = last - 1; p0 > first; p0 -= 64) {
                int p = p0 - lane;
                bool stop = (p > first) && !less(pv, a[p]);
                uint64_t mk = __ballot(stop);
                if (stop) dl[nd + popc64(mk & lt)] = (uint16_t)p;
                nd += popc64(mk);
            }
            if (lane == 0) dl[nd] = (uint16_t)first;   // the pivot itself stops the down-scan
            WAVE_SYNC();
            int k = 0;
            {
                const int tmax = nu < nd ? nu : nd;
                bool open = true;
                for (int t0 = 0; t0 < tmax && open; t0 += 64) {
                    int t = t0 + lane;
                    bool ok = (t < tmax) && (ul[t] < dl[t]);
                    uint64_t mk = __ballot(ok);
                    uint64_t inv = ~mk;
                    int run = inv ? __builtin_ctzll(inv) : 64;
                    k += run;
                    open = (run == 64);
                }
            }
            T xu, xd;
            for (int t0 = 0; t0 < k; t0 += 64) {
                int t = t0 + lane;
                if (t < k) { xu = a[ul[t]]; xd = a[dl[t]]; }
                WAVE_SYNC();
                if (t < k) { a[ul[t]] = xd; a[dl[t]] = xu; }
                WAVE_SYNC();
            }
            int cut;
            {
                int cu = (k < nu) ? (int)ul[k] : 0x7FFFFFFF;
                int cd = (k > 0) ? (int)dl[k - 1] : 0x7FFFFFFF;
                cut = cu < cd ? cu : cd;
            }
            WAVE_SYNC();
            if (lane == 0) {
                // [first, cut) and [cut, last): longer than 16 -> next level, else a final segment (marked at its start)
                if (cut - first > 16) { const int qi = atomicAdd(&qcnt[cur ^ 1], 1); qout[3 * qi] = first; qout[3 * qi + 1] = cut; qout[3 * qi + 2] = depth; }
                else atomicOr(&segmark[first >> 5], 1u << (first & 31));
                if (last - cut > 16) { const int qi = atomicAdd(&qcnt[cur ^ 1], 1); qout[3 * qi] = cut; qout[3 * qi + 1] = last; qout[3 * qi + 2] = depth; }
                else if (cut < last) atomicOr(&segmark[cut >> 5], 1u << (cut & 31));
            }
            WAVE_SYNC();
        }
        __syncthreads();
        if (tid == 0) qcnt[cur] = 0;
        cur ^= 1;
        __syncthreads();
    }
    // final insertion sort: thread t takes the segments that start in the 32-position words t, t+NTB, ...
    for (int w0 = tid; w0 * 32 < n; w0 += NTB) {
        uint32_t bits = segmark[w0];
        while (bits) {
            const int s0 = w0 * 32 + __builtin_ctz(bits);
            bits &= bits - 1;
            int e0 = n;
            if (bits) e0 = w0 * 32 + __builtin_ctz(bits);
            else {
                for (int w1 = w0 + 1; w1 * 32 < n; ++w1) { uint32_t bb = segmark[w1]; if (bb) { e0 = w1 * 32 + __builtin_ctz(bb); break; } }
            }
            if (e0 > n) e0 = n;
            for (int i = s0 + 1; i < e0; ++i) {
                T v = a[i];
                int j = i - 1;
                while (j >= s0 && less(v, a[j])) { a[j + 1] = a[j]; --j; }
                a[j + 1] = v;
            }
        }
    }
    __syncthreads();
}

// Long surviving columns with several waves per column: gather (all threads, traversal order kept by a prefix count), sort by
// id, merge, order by o_n, store -- the two sorts are block_std_sort.  NW waves, records + stop lists + segment queues in
// dynamic LDS: lcap * 16 + 2 * (lcap + 2) * 2 + 2 * 3 * QCAP * 4 bytes.
template <int NW>
__global__ __launch_bounds__(NW * 64) void k_sc_merge_mw(Arrays A, const GraphDesc* __restrict__ gd, const int32_t* __restrict__ vgraph,
                                                          const uint32_t* __restrict__ order, const int32_t* __restrict__ ext,
                                                          const int64_t* __restrict__ tmp_off, const int32_t* __restrict__ list,
                                                          const int32_t* __restrict__ count, int32_t* __restrict__ tmp_nbr,
                                                          double* __restrict__ tmp_val, int32_t* __restrict__ cnt_out,
                                                          unsigned long long* __restrict__ live_total, int32_t lcap, int32_t qcap) {
    constexpr int NTB = NW * 64;
    extern __shared__ Rec2 R_mw[];
    Rec2* const R = R_mw;
    uint16_t* const ulist = reinterpret_cast<uint16_t*>(R + lcap);
    uint16_t* const dlist = ulist + (lcap + 2);
    int32_t* const segq = reinterpret_cast<int32_t*>(dlist + (lcap + 2));   // (lcap is even: 4-byte aligned)
    __shared__ uint32_t s_segmark[BIGCAP / 32 + 2];
    __shared__ int32_t s_qcnt[2];
    __shared__ int32_t s_seg_base[40], s_seg_first[40], s_seg_pref[41], s_nseg;   // the column as runs of slots in traversal order
    __shared__ int32_t s_wtot[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t lt = lanemask_lt(lane);
    const int32_t nbig = *count;
    unsigned long long live_acc = 0ull;
    for (int32_t bi = blockIdx.x; bi < nbig; bi += gridDim.x) {
        const int32_t i = list[bi];
        const int32_t v = (int32_t)order[i];
        const int64_t toff = tmp_off[i];
        if (tid == 0) {
            // traversal order (:248-271): appended chunks newest first (each backwards), then the CSR segment backwards
            const int32_t cp0 = A.colptr[v], cp1 = A.colptr[v + 1];
            const int32_t acnt = A.vr[v].app_cnt;
            int ns = 0, pref = 0;
            int32_t idx = acnt - 1, base = A.vr[v].app_chunk;
            int c = idx >= 0 ? chunk_of(idx) : 0;
            while (idx >= 0) {
                const int32_t cs = chunk_start(c);
                s_seg_base[ns] = base + 1; s_seg_first[ns] = idx - cs;   // slot of traversal position 0 of this run = base + 1 + (idx - cs), then descending
                s_seg_pref[ns] = pref; pref += idx - cs + 1; ++ns;
                const int32_t prev = A.e[base].nbr;
                idx = cs - 1; base = prev; --c;
            }
            s_seg_base[ns] = cp0; s_seg_first[ns] = cp1 - 1 - cp0; s_seg_pref[ns] = pref; pref += cp1 - cp0; ++ns;
            s_seg_pref[ns] = pref;
            s_nseg = ns;
        }
        __syncthreads();
        const int32_t extv = s_seg_pref[s_nseg];
        int32_t len0 = 0;
        for (int32_t e0 = 0; e0 < extv; e0 += NTB) {
            const int32_t e = e0 + tid;
            double val = 0; int32_t nb = 0;
            if (e < extv) {
                int sgi = 0;
                while (e >= s_seg_pref[sgi + 1]) ++sgi;
                const int32_t sl = s_seg_base[sgi] + s_seg_first[sgi] - (e - s_seg_pref[sgi]);
                const Slot g = A.e[sl]; val = g.val; nb = g.nbr;
            }
            const bool live = e < extv && val > 0;
            const uint64_t mask = __ballot(live);
            if (lane == 0) s_wtot[wave] = popc64(mask);
            __syncthreads();
            int32_t before = len0, tot = 0;
            for (int w = 0; w < NW; ++w) { const int32_t t = s_wtot[w]; if (w < wave) before += t; tot += t; }
            if (live) { Rec2 r; r.a = (double)nb; r.b = val; R[before + popc64(mask & lt)] = r; }
            len0 += tot;
            __syncthreads();
        }
        // sort by id (:314-315)
        block_std_sort<Rec2, Rec2LessA, NW>(R, len0, Rec2LessA(), ulist, dlist, s_segmark, segq, s_qcnt, qcap);
        // merge (:317-329), NTB positions at a time: heads by comparison with the predecessor, sums in sorted order; all reads of a
        // block (its look-ahead included) come before its writes, which land at or below the block
        int32_t m = 0;
        for (int32_t p0 = 0; p0 < len0; p0 += NTB) {
            const int32_t p = p0 + tid;
            const bool act = p < len0;
            Rec2 me = {0.0, 0.0};
            double prev = -1.0;
            if (act) { me = R[p]; if (p > 0) prev = R[p - 1].a; }
            const bool head = act && me.a != prev;
            if (head) for (int32_t q = p + 1; q < len0 && R[q].a == me.a; ++q) me.b += R[q].b;
            const uint64_t mask = __ballot(head);
            if (lane == 0) s_wtot[wave] = popc64(mask);
            __syncthreads();
            int32_t before = m, tot = 0;
            for (int w = 0; w < NW; ++w) { const int32_t t = s_wtot[w]; if (w < wave) before += t; tot += t; }
            if (head) R[before + popc64(mask & lt)] = me;
            m += tot;
            __syncthreads();
        }
        // order by o_n (:331-343)
        with_rec2_order(A, gd, vgraph, v, [&](auto less) { block_std_sort<Rec2, decltype(less), NW>(R, m, less, ulist, dlist, s_segmark, segq, s_qcnt, qcap); });
        for (int32_t j = tid; j < m; j += NTB) { tmp_nbr[toff + j] = (int32_t)R[j].a; tmp_val[toff + j] = R[j].b; }
        if (tid == 0) { cnt_out[i] = m; live_acc += (unsigned long long)len0; }
        __syncthreads();
    }
    if (tid == 0 && live_acc) atomicAdd(live_slot(live_total), live_acc);
}

__global__ __launch_bounds__(64) void k_sc_merge_huge(Arrays A, const GraphDesc* __restrict__ gd, const int32_t* __restrict__ vgraph,
                                                      const uint32_t* __restrict__ order, const int32_t* __restrict__ ext,
                                                      const int64_t* __restrict__ tmp_off, const int32_t* __restrict__ list,
                                                      const int32_t* __restrict__ count, int32_t* __restrict__ tmp_nbr,
                                                      double* __restrict__ tmp_val, int32_t* __restrict__ cnt_out,
                                                      unsigned long long* __restrict__ live_total, uint16_t* __restrict__ lists,
                                                      SRec* __restrict__ scratch, unsigned long long* __restrict__ scratch_top, int64_t scratch_cap,
                                                      int32_t* __restrict__ flags) {
    static_assert(sizeof(Rec2) == sizeof(SRec), "the long-column records borrow the output pass's record scratch");
    sc_merge_long_body<true>(A, gd, vgraph, order, ext, tmp_off, list, count, tmp_nbr, tmp_val, cnt_out, live_total, lists, nullptr, 0,
                             reinterpret_cast<Rec2*>(scratch), scratch_top, scratch_cap, flags);
}

// Pass B (the prefix-sum compaction): row r of the output belongs to the surviving vertex i with
// row_off[i] <= r < row_off[i+1].  One lane per ROW (tiles of 64 consecutive rows per wave, a
// contiguous run of tiles per wave), so lanes stay busy whatever the column lengths are; the
// owner of each row is found in the tile's window of row_off by a 6-step search over lane
// registers, and the 64x3 doubles are staged through LDS so that every store is a contiguous
// 512-byte wave store.  id_mod > 0 (views call): view k's global ids [k N, (k+1) N) go back to the input's [0, N) (N = id_mod);
// 0 = ids as they are.  row_base (depths call): the rows go behind the *row_base rows of the earlier snapshots; nullptr = 0.
__global__ __launch_bounds__(256) void k_sc_compact(const uint32_t* __restrict__ order, const int32_t* __restrict__ cnt,
                                                    const int64_t* __restrict__ row_off, const int64_t* __restrict__ tmp_off,
                                                    const int32_t* __restrict__ tmp_nbr, const double* __restrict__ tmp_val,
                                                    int32_t S, double* __restrict__ out, int64_t out_cap, int32_t id_mod,
                                                    const int64_t* __restrict__ row_base) {
    (void)cnt;
    if (row_base) { const int64_t b = *row_base; out += 3 * b; out_cap -= b; }
    __shared__ double stage[4][192];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t m_total = row_off[S];
    if (m_total > out_cap) return;   // the caller's buffer is too small: nothing is written, the row count is reported
    const int64_t ntiles = (m_total + 63) >> 6;
    const int64_t per = (ntiles + nwaves - 1) / nwaves;
    int64_t t0 = wave * per, t1 = t0 + per;
    if (t1 > ntiles) t1 = ntiles;
    if (t0 >= t1) return;
    // owner of the first row of this wave's run: last i with row_off[i] <= r
    int32_t i0;
    {
        const int64_t r = t0 << 6;
        int32_t lo = 0, hi = S;   // invariant: row_off[lo] <= r < row_off[hi] (row_off[S] = m_total > r)
        while (hi - lo > 1) {
            int32_t mid = (lo + hi) >> 1;
            if (row_off[mid] <= r) lo = mid; else hi = mid;
        }
        i0 = lo;
    }
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t r = (t << 6) + lane;
        const bool valid = r < m_total;
        int32_t owner = i0;
        int64_t obase = 0;
        // window search; windows advance by 63 while some lane's row lies beyond the window
        int32_t wbase = i0;
        bool found = false;
        while (true) {
            int32_t idx = wbase + lane;
            int64_t ro = row_off[idx <= S ? idx : S];
            // largest p in [0,63] with ro_p <= r
            int p = 0;
#pragma unroll
            for (int step = 32; step > 0; step >>= 1) {
                int q = p + step;
                int64_t rq = __shfl(ro, q);
                if (rq <= r) p = q;
            }
            int64_t rp = __shfl(ro, p);
            bool inside = (p < 63) || (wbase + 63 >= S);   // p == 63 may mean "further right"
            if (!found && (inside || !valid)) { owner = wbase + p; obase = rp; found = true; }
            if (__ballot(!found) == 0ull) break;
            wbase += 63;
        }
        if (owner >= S) owner = S - 1;
        double f0 = 0, f1 = 0, f2 = 0;
        if (valid) {
            const int64_t src = tmp_off[owner] + (r - obase);
            int32_t a = tmp_nbr[src];
            uint32_t b = order[owner];
            if (id_mod > 0) {   // (edges never cross views: the owner's view is the neighbour's, one division per row)
                const uint32_t sh = (b / (uint32_t)id_mod) * (uint32_t)id_mod;
                a -= (int32_t)sh; b -= sh;
            }
            f0 = (double)a;
            f1 = (double)b;
            f2 = tmp_val[src];
        }
        double* st = stage[wv];
        st[lane * 3 + 0] = f0; st[lane * 3 + 1] = f1; st[lane * 3 + 2] = f2;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int64_t o0 = (t << 6) * 3;
        const int64_t lim = m_total * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int64_t d = o0 + lane + 64 * k;
            if (d < lim) out[d] = st[lane + 64 * k];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        i0 = __shfl(owner, 63);
    }
}

// per-graph row pointers: first output position of each graph
__global__ void k_graph_rows(const int64_t* __restrict__ surv_base, const int64_t* __restrict__ row_off, int32_t G, int64_t* __restrict__ out_ptr) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > G) return;
    out_ptr[g] = row_off[surv_base[g]];
}

}  // namespace rlap
