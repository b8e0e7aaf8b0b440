// rlap_kernels.hip -- the round kernels of the rLap augmentor, hand-written for gfx950 (wave64).
//
//   K5-K8 k_eliminate_batch_t<o_v,o_n,slots,threads>  one workgroup per graph, rounds of independent
//                            vertices with exact sequential semantics; wave_eliminate / wave_eliminate_big /
//                            serial_eliminate for what a round cannot take
//                            (preconditioner.cc:348-433 | 713-787 | 835-914)
//   k_eq_tables, launch_eliminate_batch / launch_eliminate_pq   the equal-key tables and the launchers
//
// The other kernels of the call have translation units of their own, so that nothing but this file and its headers decides the
// round kernels' machine code (an out-of-line device function is compiled once for all its callers in a unit):
//   K10, K1-K4               rlap_setup.hip     sampling stream, COO -> CSR, twin check, bucket queue, views
//   K9                       rlap_output.hip    output pass (k_sc_*)
//   k_debug_wave_sort        rlap_sorthook.hip  test hook of the sorts in rlap_wave_sort.h
//
// Compiled with -ffp-contract=off: the reference is built without FMA
// (setup.py:26-37), and index selection depends on the exact roundings.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdlib>
#include <type_traits>

#include "rlap_core.h"
#include "rlap_kernels.h"
#include "rlap_wave_sort.h"

namespace rlap {


// This file is compiled twice (Makefile).  rlap_kernels.o has the o_v = random instantiations of the elimination kernel, the
// equal-key tables and the launchers; rlap_kernels_pq.o (-DRLAP_ELIM_PQ_TU -mllvm -disable-machine-licm) has the priority-queue instantiations and their launcher: with machine LICM the invariants that get
// hoisted out of the round loop (LDS base addresses, the reciprocal of n, pointers moved to VGPRs) are spilled in its preheader and
// reloaded from scratch inside it -- 79 reloads in <degree,asc,32,1024>, 12 without; the o_v = random kernels are better off with it.
// ---------------------------------------------------------------------------
// K5-K8: elimination.  One 1024-thread workgroup per graph runs rounds of the batch
// ("frontier") scheme; vertices it cannot take (long columns, multi-edges, keys
// beyond n) go through the single-vertex wave path or the sequential fallback.
// ---------------------------------------------------------------------------



template <int EC>
struct ElimLdsT {
    SRec rec[EC];  // sort records; after ordering re-used as cum[EC] + newv[EC]
    double a_val[EC];
    double b_val[EC];
    int32_t a_slot[EC], a_nbr[EC], a_twin[EC];
    int32_t b_slot[EC], b_nbr[EC], b_twin[EC], b_pos[EC], b_dup[EC];
    int32_t ksel[EC], t_key[EC], t_mv[EC], t_of[EC], t_cnt[EC], t_chunk[EC], t_list[EC], t_rank[EC], pslot[EC];
    WaveSortScratchT<EC> ws;
    alignas(16) double skey[EC + 8];   // sort keys as staged (kept: a sort that meets the depth limit starts over from them)
};

// std::sort order of the staged keys L.skey[0..cnt) into L.rec[] = {key, source index}: one element per lane
// up to 64 keys, the level-synchronous introsort restatement beyond.
template <bool GREATER, int EC>
__device__ __forceinline__ void wave_sort_staged(ElimLdsT<EC>& L, int cnt, int lane) {
    if (cnt <= 64) {
        double key = lane < cnt ? L.skey[lane] : 0.0;
        int idx = lane, pos = lane;
        const bool ok = wave_sort64<GREATER>(key, idx, cnt, lane, L.pslot, &pos);   // pslot is free until the slots are handed out
        if (ok) {
            if (lane < cnt) { L.rec[pos].key = key; L.rec[pos].idx = idx; }
            WAVE_SYNC();
            return;
        }
    }
    WAVE_SYNC();
    const WaveSortPtrs WP = {L.ws.ulist, L.ws.dlist, L.ws.segmark, L.ws.stk};
    for (int i = lane; i < cnt; i += 64) { L.rec[i].key = L.skey[i]; L.rec[i].idx = i; }
    WAVE_SYNC();
    // beyond 64 keys: the introsort restatement, one pass per recursion level (wave_lvl_sort; exact with or without ties -- a
    // stable rank costs as much and is only exact without them); its depth-limit exit starts over.  t_rank / pslot are free here.
    typedef typename std::conditional<GREATER, SRecGreaterKey, SRecLessKey>::type Cmp;
    bool ok;
    if (cnt <= 128) ok = wave_lvl_sort<SRec, Cmp, 2>(L.rec, cnt, Cmp(), L.ws.ulist, L.ws.dlist, reinterpret_cast<uint32_t*>(L.t_rank), reinterpret_cast<uint16_t*>(L.pslot), lane);
    else if (cnt <= 256) ok = wave_lvl_sort<SRec, Cmp, 4>(L.rec, cnt, Cmp(), L.ws.ulist, L.ws.dlist, reinterpret_cast<uint32_t*>(L.t_rank), reinterpret_cast<uint16_t*>(L.pslot), lane);
    else ok = wave_lvl_sort<SRec, Cmp, EC / 64>(L.rec, cnt, Cmp(), L.ws.ulist, L.ws.dlist, reinterpret_cast<uint32_t*>(L.t_rank), reinterpret_cast<uint16_t*>(L.pslot), lane);
    if (!ok) {
        WAVE_SYNC();
        for (int i = lane; i < cnt; i += 64) { L.rec[i].key = L.skey[i]; L.rec[i].idx = i; }
        WAVE_SYNC();
        wave_std_sort<SRec, Cmp, EC / 64>(L.rec, cnt, Cmp(), WP, lane);
    }
    WAVE_SYNC();
}

__device__ __forceinline__ int32_t alloc_in_column(const Arrays& A, int32_t& a, int32_t& chunk, int32_t* status) {
    int c = chunk_of(a);
    int cs = chunk_start(c);
    if (a == cs) {
        int32_t need = 1 + chunk_cap(c);
        int32_t base = atomicAdd(A.pool_top, need);
        if (base < 0 || base > A.slot_cap - need) { *status = ST_POOL_OVERFLOW; return 0; }
        A.e[base].nbr = chunk;
        chunk = base;
    }
    int32_t s = chunk + 1 + (a - cs);
    a += 1;
    return s;
}

__device__ __forceinline__ int32_t ld_agent(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The f / colScale / wdeg recurrence (:396-417): new weight of every position but the last.  One lane; the operation order is the result.
template <int EC>
__device__ __forceinline__ void new_weights(const double* a_val, double* newv, int m, double csum) {
    double wdeg = csum, colScale = 1;
    for (int j0 = 0; j0 < m - 1; j0 += 8) {
        double vv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) vv[u] = a_val[j0 + u < EC ? j0 + u : EC - 1];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (j0 + u < m - 1) {
                double w = vv[u] * colScale;
                double f = w / wdeg;
                double omf = 1 - f;
                newv[j0 + u] = f * omf * wdeg;
                colScale = colScale * omf;
                wdeg = wdeg * omf * omf;
            }
        }
    }
}

constexpr int SPIN_LIMIT = 1 << 26;   // s_sleep(1) rounds a wave waits for another one of its workgroup before it gives up with ST_INTERNAL (about 2 s: the
                                      // helper wave also sits out the sequential fall-back of a very long column, tens of milliseconds)
constexpr int HELP_MIN = 24;   // columns shorter than this keep the recurrence on the eliminating wave (the hand-over costs about a microsecond)

// Wave 1 while wave 0 runs the single-vertex path: waits for the request, runs the recurrence over the ordered weights, reports.
// (csum is recomputed here: the same left-to-right sum the eliminating wave forms for the cumulative weights.)
template <int EC>
__device__ __noinline__ void single_helper(ElimLdsT<EC>& L, double* big_newv, int32_t* help) {
    const int lane = lane_id();
    int f = 0;
    if (lane == 0) {
        int sp = 0;
        while ((f = __hip_atomic_load(&help[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) != 1 && f != 3 && f != 4 && ++sp < SPIN_LIMIT) __builtin_amdgcn_s_sleep(1);
        if (sp >= SPIN_LIMIT) help[2] = 1;   // gave up: the workgroup reports ST_INTERNAL (a request posted later would never be answered)
    }
    f = __shfl(f, 0);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (f == 4) {   // the long-column path (wave_eliminate_big): the ordered weights are in its newv[], rewritten in place
        if (lane == 0) {
            const int m = help[1];
            double csum = 0;
            for (int j = 0; j < m; ++j) csum += big_newv[j];
            double wdeg = csum, colScale = 1;
            for (int j = 0; j < m - 1; ++j) {
                double w = big_newv[j] * colScale;
                double f2 = w / wdeg;
                double omf = 1 - f2;
                big_newv[j] = f2 * omf * wdeg;
                colScale = colScale * omf;
                wdeg = wdeg * omf * omf;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __hip_atomic_store(&help[0], 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        return;
    }
    if (f != 1) {
        if (lane == 0 && f == 3) __hip_atomic_store(&help[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return;
    }
    if (lane == 0) {
        const int m = help[1];
        double csum = 0;
        for (int j0 = 0; j0 < m; j0 += 8) {
            double vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) vv[u] = L.a_val[j0 + u < EC ? j0 + u : EC - 1];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (j0 + u < m) csum += vv[u];
        }
        new_weights<EC>(L.a_val, reinterpret_cast<double*>(L.rec) + EC, m, csum);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __hip_atomic_store(&help[0], 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// Single-vertex path, executed by ONE wave (columns up to EC entries, multi-edges, any key range).
template <int EC>
__device__ __noinline__ void wave_eliminate(const Arrays& A, GraphDesc& G, ElimLdsT<EC>& L, int32_t v, int64_t e1, int32_t cp0, int32_t cp1,
                               int32_t acnt, int32_t abase, long long* wprof, int32_t* help) {
    const int lane = lane_id();
    long long wt_prev = wprof ? wall_clock64() : 0;
#define WSTAMP(k) do { if (wprof && lane == 0) { long long _t = wall_clock64(); wprof[k] += _t - wt_prev; wt_prev = _t; } } while (0)
    const bool use_pq = A.o_v != OV_RANDOM;
    const bool coarsen = A.o_v == OV_COARSEN;
    const uint64_t lt = lanemask_lt(lane);

    // ---- gather live entries in the reference's traversal order (:248-271) ----
    int len0 = 0;
    {
        int32_t idx = acnt - 1, base = abase;
        int c = idx >= 0 ? chunk_of(idx) : 0;
        while (idx >= 0) {
            int32_t cs = chunk_start(c);
            for (int32_t t0 = idx; t0 >= cs; t0 -= 64) {
                int32_t t = t0 - lane;
                bool valid = t >= cs;
                int32_t s = base + 1 + (t - cs);
                double val = 0; int32_t nb = 0, tw = 0;
                if (valid) { const Slot g = A.e[s]; val = g.val; nb = g.nbr; tw = g.twin; }
                bool live = valid && val > 0;
                uint64_t mask = __ballot(live);
                int pos = len0 + popc64(mask & lt);
                if (live) { L.a_slot[pos] = s; L.a_nbr[pos] = nb; L.a_val[pos] = val; L.a_twin[pos] = tw; }
                len0 += popc64(mask);
            }
            int32_t prev = A.e[base].nbr;
            idx = cs - 1; base = prev; --c;
        }
        for (int32_t s0 = cp1 - 1; s0 >= cp0; s0 -= 64) {
            int32_t s = s0 - lane;
            bool valid = s >= cp0;
            double val = 0; int32_t nb = 0, tw = 0;
            if (valid) { const Slot g = A.e[s]; val = g.val; nb = g.nbr; tw = g.twin; }
            bool live = valid && val > 0;
            uint64_t mask = __ballot(live);
            int pos = len0 + popc64(mask & lt);
            if (live) { L.a_slot[pos] = s; L.a_nbr[pos] = nb; L.a_val[pos] = val; L.a_twin[pos] = tw; }
            len0 += popc64(mask);
        }
    }
    WAVE_SYNC();
    WSTAMP(0);

    // ---- sort by neighbour id (std::sort semantics, :275-276) ----
    for (int i = lane; i < len0; i += 64) L.skey[i] = (double)L.a_nbr[i];
    WAVE_SYNC();
    wave_sort_staged<false>(L, len0, lane);

    WSTAMP(1);
    // ---- merge multi-edges (:278-293) ----
    int m = 0;
    if (len0 <= 64) {
        bool act = lane < len0;
        int src = act ? L.rec[lane].idx : 0;
        int32_t nb = act ? L.a_nbr[src] : -1;
        int32_t nbprev = __shfl_up(nb, 1);
        bool head = act && (lane == 0 || nb != nbprev);
        uint64_t mask = __ballot(head);
        m = popc64(mask);
        int x = popc64(mask & (lt | (1ull << lane))) - 1;
        if (head) {
            uint64_t above = (lane == 63) ? 0ull : (mask >> (lane + 1));
            int nexthead = above ? (lane + 1 + __builtin_ctzll(above)) : len0;
            int d = nexthead - lane - 1;
            double val = L.a_val[src];
            for (int q = 1; q <= d; ++q) val += L.a_val[L.rec[lane + q].idx];
            L.b_slot[x] = L.a_slot[src]; L.b_nbr[x] = nb; L.b_twin[x] = L.a_twin[src]; L.b_val[x] = val;
            L.b_pos[x] = lane; L.b_dup[x] = d;
        } else if (act) {
            A.e[L.a_twin[src]].val = 0;  // duplicate's twin dies (:289)
        }
    } else {
        for (int p0 = 0; p0 < len0; p0 += 64) {
            const int p = p0 + lane;
            const bool act = p < len0;
            const int src = act ? L.rec[p].idx : 0;
            const int32_t nb = act ? L.a_nbr[src] : -1;
            const int32_t nbprev = (act && p > 0) ? L.a_nbr[L.rec[p - 1].idx] : -2;
            const bool head = act && nb != nbprev;
            const uint64_t mask = __ballot(head);
            const int x = m + popc64(mask & lt);
            if (head) {
                double val = L.a_val[src];
                int d = 0;
                for (int q = p + 1; q < len0 && L.a_nbr[L.rec[q].idx] == nb; ++q) { val += L.a_val[L.rec[q].idx]; ++d; }
                L.b_slot[x] = L.a_slot[src]; L.b_nbr[x] = nb; L.b_twin[x] = L.a_twin[src]; L.b_val[x] = val;
                L.b_pos[x] = p; L.b_dup[x] = d;
            } else if (act) {
                A.e[L.a_twin[src]].val = 0;  // duplicate's twin dies (:289)
            }
            m += popc64(mask);
        }
    }
    WAVE_SYNC();

    WSTAMP(2);
    // ---- neighbour metadata (PQ key, append cursor): issued now, used after ordering ----
    for (int x = lane; x < m; x += 64) {
        int32_t nb = L.b_nbr[x];
        L.t_cnt[x] = A.vr[nb].app_cnt;
        L.t_chunk[x] = A.vr[nb].app_chunk;
        L.t_key[x] = use_pq ? A.vr[nb].key : 0;
    }

    // ---- order neighbours by o_n (:295-307) ----
    {
        if (A.o_n == ON_RANDOM || coarsen) {
            uint64_t kb = keyed_order_base(A.shuffle_seed, v - G.vbase, 0);
            for (int i = lane; i < m; i += 64) L.skey[i] = keyed_order_dkey(kb, L.b_nbr[i] - G.vbase);
            WAVE_SYNC();
            wave_sort_staged<false>(L, m, lane);
        } else {
            for (int i = lane; i < m; i += 64) L.skey[i] = L.b_val[i];
            WAVE_SYNC();
            if (A.o_n == ON_ASC) wave_sort_staged<false>(L, m, lane);
            else wave_sort_staged<true>(L, m, lane);
        }
        for (int j = lane; j < m; j += 64) {
            int x = L.rec[j].idx;
            L.t_of[j] = x;
            L.a_slot[j] = L.b_slot[x]; L.a_nbr[j] = L.b_nbr[x]; L.a_val[j] = L.b_val[x]; L.a_twin[j] = L.b_twin[x];
        }
    }
    WAVE_SYNC();

    WSTAMP(3);
    double* cum = reinterpret_cast<double*>(L.rec);
    double* newv = cum + EC;
    int32_t status = 0;
    int koff_c = 0;        // coarsen: chosen position
    double wk_c = 0;

    // ---- cumulative weights + the f / colScale / wdeg recurrences (:366-417) ----
    // The second recurrence (the new weights) is not needed before the rewire: wave 1 of the workgroup, idle otherwise, runs it
    // (single_helper) while this wave samples and hands out the slots.  help[0]: 0 idle, 1 request (help[1] = m), 2 done, 3 no request.
    const bool helped = !coarsen && m >= HELP_MIN;
    if (helped && lane == 0) {
        help[1] = m;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __hip_atomic_store(&help[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    // (a wait that runs out is an internal error, never a result: the new weights would be read unfinished)
#define HELP_FINISH() do { if (helped) { if (lane == 0) { int _sp = 0; while (__hip_atomic_load(&help[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 2 && ++_sp < SPIN_LIMIT) __builtin_amdgcn_s_sleep(1); \
        if (_sp >= SPIN_LIMIT) G.status = ST_INTERNAL; \
        __hip_atomic_store(&help[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); } __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); WAVE_SYNC(); } \
        else if (lane == 0) __hip_atomic_store(&help[0], 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); } while (0)
    if (lane == 0) {
        // the two recurrences are the result's operation order: one lane, values fetched eight at a time
        // (nothing else runs on the CU now, so every LDS round trip would be waited for)
        double csum = 0;
        for (int j0 = 0; j0 < m; j0 += 8) {
            double vv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) vv[u] = L.a_val[j0 + u < EC ? j0 + u : EC - 1];
#pragma unroll
            for (int u = 0; u < 8; ++u) { if (j0 + u < m) { csum += vv[u]; cum[j0 + u] = csum; } }
        }
        if (!coarsen && !helped) new_weights<EC>(L.a_val, newv, m, csum);
    }
    WAVE_SYNC();
    WSTAMP(4);
    const double csum = m > 0 ? cum[m - 1] : 0.0;
    const int64_t draws0 = G.n_draws;
    int ndraw = coarsen ? (m >= 1 ? 1 : 0) : (m > 1 ? m - 1 : 0);
    if (draws0 + ndraw > A.rng_len) { HELP_FINISH(); if (lane == 0) G.status = ST_RNG_OVERFLOW; WAVE_SYNC(); return; }

    if (coarsen) {
        if (m >= 1) {
            double u = arr_uniform(A, draws0, v, 0);
            double r = u * csum;
            koff_c = upper_index(cum, m, r);
            wk_c = L.a_val[koff_c];
        }
    } else {
        // ---- sample k for every position but the last (:385-394) ----
        for (int j = lane; j < m - 1; j += 64) {
            double u = arr_uniform(A, draws0 + j, v, j);
            double cj = cum[j];
            double r = u * (csum - cj) + cj;
            L.ksel[j] = upper_index(cum, m, r);
        }
    }
    WAVE_SYNC();

    WSTAMP(5);
    // ---- per-neighbour: PQ op replay (:291,:399,:427 | :882,:896) + slots for the pushes into its column ----
    const int xk_c = (coarsen && m >= 1) ? L.t_of[koff_c] : -1;
    if (!use_pq) {
        // no PQ to replay (o_v = random): hand out the slots 64 positions at a time, in position order.  Lanes
        // that drew the same target form a group; its first lane advances the target's append cursor (kept in
        // LDS between the chunks) once per member, in lane order.
        for (int x = lane; x < m; x += 64) L.t_list[x] = L.t_cnt[x];   // cursor before this vertex
        WAVE_SYNC();
        for (int j0 = 0; j0 < m - 1; j0 += 64) {
            const int j = j0 + lane;
            const bool act = j < m - 1;
            const int x = act ? L.t_of[L.ksel[j]] : 0;
            uint64_t mymask = __ballot(act);   // lanes that drew my target: one ballot per bit of its index (< EC <= 512)
            static_assert(EC <= 512 && EC % 64 == 0, "9 bits of target index");
#pragma unroll
            for (int bit = 0; bit < 9; ++bit) {
                const bool mybit = (x >> bit) & 1;
                const uint64_t bb = __ballot(act && mybit);
                mymask &= mybit ? bb : ~bb;
            }
            if (act && lane == __builtin_ctzll(mymask)) {
                int32_t a = L.t_cnt[x], chunk = L.t_chunk[x];
                uint64_t mm = mymask;
                while (mm) { const int l = __builtin_ctzll(mm); mm &= mm - 1; L.t_rank[l] = alloc_in_column(A, a, chunk, &status); }
                L.t_cnt[x] = a; L.t_chunk[x] = chunk;
            }
            WAVE_SYNC();
            if (act) L.pslot[j] = L.t_rank[lane];
            WAVE_SYNC();
        }
        for (int x = lane; x < m; x += 64) {
            if (L.t_cnt[x] != L.t_list[x]) { A.vr[L.b_nbr[x]].app_cnt = L.t_cnt[x]; A.vr[L.b_nbr[x]].app_chunk = L.t_chunk[x]; }
        }
    } else
    for (int x = lane; x < m; x += 64) {
        int key = L.t_key[x], mv = -1;
        int32_t a = L.t_cnt[x], chunk = L.t_chunk[x];
        const int32_t a_before = a;
        if (use_pq) {
            int d = L.b_dup[x], p0 = L.b_pos[x];
            for (int q = 1; q <= d; ++q) pq_op(key, mv, G.n, -1, p0 + q);
        }
        if (coarsen) {
            if (x == xk_c) {
                pq_op(key, mv, G.n, -1, len0);
                for (int j = 0; j < m; ++j) {
                    if (j == koff_c) continue;
                    pq_op(key, mv, G.n, +1, len0 + 1 + j);
                    L.pslot[j] = alloc_in_column(A, a, chunk, &status);
                }
            }
        } else {
            for (int j = 0; j < m - 1; ++j) {
                if (L.t_of[L.ksel[j]] == x) {
                    if (use_pq) pq_op(key, mv, G.n, +1, len0 + j);
                    L.pslot[j] = alloc_in_column(A, a, chunk, &status);
                }
            }
            if (use_pq && x == L.t_of[m - 1] && e1 + 1 < (int64_t)G.n) pq_op(key, mv, G.n, -1, len0 + m);
        }
        if (a != a_before) { A.vr[L.b_nbr[x]].app_cnt = a; A.vr[L.b_nbr[x]].app_chunk = chunk; }
        if (use_pq) {
            if (key != L.t_key[x]) A.vr[L.b_nbr[x]].key = key;
            L.t_key[x] = key;
            L.t_mv[x] = mv;
            L.t_list[x] = mv >= 0 ? pq_list_of(key, G.n) : -1;
        }
    }
    HELP_FINISH();   // (the new weights are in place from here on)
    if (__ballot(status != 0) != 0ull) { if (lane == 0) G.status = ST_POOL_OVERFLOW; WAVE_SYNC(); return; }
    WAVE_SYNC();

    WSTAMP(6);
    // ---- rewire: twin rewritten in place, new entry appended to column k (:404-414) ----
    if (coarsen) {
        for (int j = lane; j < m; j += 64) {
            if (j == koff_c) continue;
            double w = L.a_val[j];
            double nw = (wk_c * w) / (wk_c + w);
            int32_t k = L.a_nbr[koff_c], s_r = L.a_twin[j], s_n = L.pslot[j];
            A.e[s_r].nbr = k; A.e[s_r].val = nw; A.e[s_r].twin = s_n;
            A.e[s_n].nbr = L.a_nbr[j]; A.e[s_n].val = nw; A.e[s_n].twin = s_r;
        }
        if (lane == 0 && m >= 1) A.e[L.a_twin[koff_c]].val = 0;
    } else {
        for (int j = lane; j < m - 1; j += 64) {
            double nw = newv[j];
            int32_t k = L.a_nbr[L.ksel[j]], s_r = L.a_twin[j], s_n = L.pslot[j];
            A.e[s_r].nbr = k; A.e[s_r].val = nw; A.e[s_r].twin = s_n;
            A.e[s_n].nbr = L.a_nbr[j]; A.e[s_n].val = nw; A.e[s_n].twin = s_r;
        }
        if (lane == 0 && m >= 1) A.e[L.a_twin[m - 1]].val = 0;  // :429-430
    }

    WSTAMP(7);
    // ---- PQ commit: moved neighbours re-enter their bucket at the head, in op order ----
    if (use_pq) {
        for (int x = lane; x < m; x += 64) {
            int mvx = L.t_mv[x];
            int rank = -1;
            if (mvx >= 0) {
                rank = 0;
                for (int y = 0; y < m; ++y) { int mvy = L.t_mv[y]; rank += (mvy >= 0 && mvy < mvx) ? 1 : 0; }
            }
            L.t_rank[x] = rank;
        }
        WAVE_SYNC();
        for (int x = lane; x < m; x += 64) { int r = L.t_rank[x]; if (r >= 0) L.pslot[r] = x; }   // pslot is free now
        int nmoved_part = 0;
        for (int x = lane; x < m; x += 64) nmoved_part += (L.t_rank[x] >= 0) ? 1 : 0;
        int nmoved = nmoved_part;
        for (int off = 32; off > 0; off >>= 1) nmoved += __shfl_xor(nmoved, off);
        WAVE_SYNC();
        if (lane == 0) {
            for (int r = 0; r < nmoved; ++r) {
                int x = L.pslot[r];
                int rc = pq_push(A, G, L.b_nbr[x], L.t_list[x]);
                if (rc) { G.status = rc; break; }
            }
        }
        WAVE_SYNC();
        if (G.status != 0) return;
    }
    if (lane == 0) G.n_draws = draws0 + ndraw;
    WAVE_SYNC();
    WSTAMP(8);
#undef WSTAMP
#undef HELP_FINISH
}


// ---------------------------------------------------------------------------
// Single-vertex path for columns beyond ECAP entries, o_v = random (hubs met early in a random order;
// no PQ to replay).  One wave; the sort records, the stop lists and afterwards the cumulative weights live
// in the workgroup's LDS (the batch round's storage is free while a single vertex is eliminated), the column
// itself in the graph's global scratch (BIGE = 7168 entries with the 1024-thread workgroup, 1536 with the 256-thread one).  Every step is O(len/64) or the O(len log len / 64) sort; the only
// lane-serial parts are the two floating-point recurrences, whose order of operations is the result.
// Returns false (nothing changed) when the column does not fit: the caller falls back to the sequential form.
// ---------------------------------------------------------------------------
template <int BIGE>
struct BigElimLdsT {
    union {
        SRec rec[BIGE];
        struct { double cum[BIGE]; double newv[BIGE]; } c;
    };
    uint16_t ulist[BIGE + 2];
    uint16_t dlist[BIGE + 2];
    uint32_t segmark[BIGE / 32 + 2];
    int32_t stk[3 * 48];
    int32_t tmp[64];
};

template <int BIGE>
__device__ __noinline__ bool wave_eliminate_big(const Arrays& A, GraphDesc& G, BigElimLdsT<BIGE>& L, const ColBuf& B, int32_t cap, int32_t v,
                                                int32_t cp0, int32_t cp1, int32_t acnt, int32_t abase, int32_t* help) {
    const int lane = lane_id();
    const uint64_t lt = lanemask_lt(lane);
    if (cap > BIGE) cap = BIGE;

    // ---- gather live entries in the reference's traversal order (:616-639) ----
    int len0 = 0;
    {
        int32_t idx = acnt - 1, base = abase;
        int c = idx >= 0 ? chunk_of(idx) : 0;
        while (idx >= 0) {
            int32_t cs = chunk_start(c);
            for (int32_t t0 = idx; t0 >= cs; t0 -= 64) {
                int32_t t = t0 - lane;
                bool valid = t >= cs;
                int32_t s = base + 1 + (t - cs);
                double val = 0; int32_t nb = 0, tw = 0;
                if (valid) { const Slot g = A.e[s]; val = g.val; nb = g.nbr; tw = g.twin; }
                bool live = valid && val > 0;
                uint64_t mask = __ballot(live);
                int pos = len0 + popc64(mask & lt);
                if (live && pos < cap) { B.a_slot[pos] = s; B.a_nbr[pos] = nb; B.a_val[pos] = val; B.a_twin[pos] = tw; }
                len0 += popc64(mask);
            }
            int32_t prev = A.e[base].nbr;
            idx = cs - 1; base = prev; --c;
        }
        for (int32_t s0 = cp1 - 1; s0 >= cp0; s0 -= 64) {
            int32_t s = s0 - lane;
            bool valid = s >= cp0;
            double val = 0; int32_t nb = 0, tw = 0;
            if (valid) { const Slot g = A.e[s]; val = g.val; nb = g.nbr; tw = g.twin; }
            bool live = valid && val > 0;
            uint64_t mask = __ballot(live);
            int pos = len0 + popc64(mask & lt);
            if (live && pos < cap) { B.a_slot[pos] = s; B.a_nbr[pos] = nb; B.a_val[pos] = val; B.a_twin[pos] = tw; }
            len0 += popc64(mask);
        }
    }
    if (len0 > cap) return false;
    WAVE_SYNC();
    const WaveSortPtrs WP = {L.ulist, L.dlist, L.segmark, L.stk};

    // ---- sort by neighbour id (std::sort semantics, :641-644) ----
    for (int i = lane; i < len0; i += 64) { L.rec[i].key = (double)B.a_nbr[i]; L.rec[i].idx = i; L.rec[i].aux = 0; }
    WAVE_SYNC();
    wave_std_sort<SRec>(L.rec, len0, SRecLessKey(), WP, lane);
    WAVE_SYNC();

    // ---- merge multi-edges (:646-659): group heads by ballot, the sum runs in sorted order ----
    int m = 0;
    for (int p0 = 0; p0 < len0; p0 += 64) {
        const int p = p0 + lane;
        const bool act = p < len0;
        const int s = act ? L.rec[p].idx : 0;
        const int32_t nb = act ? B.a_nbr[s] : -1;
        const int32_t nbprev = (act && p > 0) ? B.a_nbr[L.rec[p - 1].idx] : -2;
        const bool head = act && nb != nbprev;
        const uint64_t mask = __ballot(head);
        const int x = m + popc64(mask & lt);
        if (head) {
            double val = B.a_val[s];
            for (int q = p + 1; q < len0 && B.a_nbr[L.rec[q].idx] == nb; ++q) val += B.a_val[L.rec[q].idx];
            B.b_slot[x] = B.a_slot[s]; B.b_nbr[x] = nb; B.b_twin[x] = B.a_twin[s]; B.b_val[x] = val;
        } else if (act) {
            A.e[B.a_twin[s]].val = 0;   // duplicate's twin dies (:655)
        }
        m += popc64(mask);
    }
    WAVE_SYNC();

    // ---- order neighbours by o_n (:661-673) ----
    if (A.o_n == ON_RANDOM) {
        const uint64_t kb = keyed_order_base(A.shuffle_seed, v - G.vbase, 0);
        for (int i = lane; i < m; i += 64) { L.rec[i].key = keyed_order_dkey(kb, B.b_nbr[i] - G.vbase); L.rec[i].idx = i; }
    } else {
        for (int i = lane; i < m; i += 64) { L.rec[i].key = B.b_val[i]; L.rec[i].idx = i; }
    }
    WAVE_SYNC();
    if (A.o_n == ON_DESC) wave_std_sort<SRec>(L.rec, m, SRecGreaterKey(), WP, lane);
    else wave_std_sort<SRec>(L.rec, m, SRecLessKey(), WP, lane);
    WAVE_SYNC();
    for (int j = lane; j < m; j += 64) {
        const int x = L.rec[j].idx;
        B.a_slot[j] = B.b_slot[x]; B.a_nbr[j] = B.b_nbr[x]; B.a_val[j] = B.b_val[x]; B.a_twin[j] = B.b_twin[x];
    }
    WAVE_SYNC();

    // ---- cumulative weights + the f / colScale / wdeg recurrences (:728-779), in LDS over the sort records ----
    double* cum = L.c.cum;
    double* newv = L.c.newv;
    for (int j = lane; j < m; j += 64) { const double w = B.a_val[j]; newv[j] = w; cum[j] = w; }
    WAVE_SYNC();
    // the new-weight recurrence runs on the workgroup's second wave (single_helper, request 4: in place over newv[]) while this
    // one forms the cumulative weights (in place over cum[]), samples and hands out the slots; it is needed at the rewire
    const bool helped = m >= HELP_MIN;
    if (helped && lane == 0) {
        help[1] = m;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __hip_atomic_store(&help[0], 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#define BIG_HELP_FINISH() do { if (helped) { if (lane == 0) { int _sp = 0; while (__hip_atomic_load(&help[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 2 && ++_sp < SPIN_LIMIT) __builtin_amdgcn_s_sleep(1); \
        if (_sp >= SPIN_LIMIT) G.status = ST_INTERNAL; \
        __hip_atomic_store(&help[0], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); } __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); WAVE_SYNC(); } \
        else if (lane == 0) __hip_atomic_store(&help[0], 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); } while (0)
    if (lane == 0) {
        double csum = 0;
        for (int j = 0; j < m; ++j) { csum += cum[j]; cum[j] = csum; }
        if (!helped) {
            double wdeg = csum, colScale = 1;
            for (int j = 0; j < m - 1; ++j) {
                double w = newv[j] * colScale;
                double f = w / wdeg;
                double omf = 1 - f;
                newv[j] = f * omf * wdeg;
                colScale = colScale * omf;
                wdeg = wdeg * omf * omf;
            }
        }
    }
    WAVE_SYNC();
    const double csum = m > 0 ? cum[m - 1] : 0.0;
    const int64_t draws0 = G.n_draws;
    const int ndraw = m > 1 ? m - 1 : 0;
    if (draws0 + ndraw > A.rng_len) { BIG_HELP_FINISH(); if (lane == 0) G.status = ST_RNG_OVERFLOW; WAVE_SYNC(); return true; }

    // ---- sample k for every position but the last (:747-756) ----
    for (int j = lane; j < m - 1; j += 64) {
        double u = arr_uniform(A, draws0 + j, v, j);
        double cj = cum[j];
        double r = u * (csum - cj) + cj;
        B.ksel[j] = upper_index(cum, m, r);
    }
    WAVE_SYNC();

    BIG_HELP_FINISH();   // (the new weights are in place from here on)
#undef BIG_HELP_FINISH
    // ---- rewire (:766-776), 64 positions at a time in position order: lanes that drew the same target form a
    //      group whose first lane hands out the target's next slots in lane (= position) order ----
    int32_t status = 0;
    for (int j0 = 0; j0 < m - 1; j0 += 64) {
        const int j = j0 + lane;
        const bool act = j < m - 1;
        const int32_t ks = act ? B.ksel[j] : 0;
        const int32_t k = act ? B.a_nbr[ks] : -1;
        uint64_t mymask = __ballot(act);   // lanes that drew my target: one ballot per bit of its position (< BIGE <= 8192)
        static_assert(BIGE <= 8192, "13 bits of target position");
#pragma unroll
        for (int bit = 0; bit < 13; ++bit) {
            const bool mybit = (ks >> bit) & 1;
            const uint64_t bb = __ballot(act && mybit);
            mymask &= mybit ? bb : ~bb;
        }
        if (act && lane == __builtin_ctzll(mymask)) {
            int32_t a = ld_agent(&A.vr[k].app_cnt), chunk = ld_agent(&A.vr[k].app_chunk);
            uint64_t mm = mymask;
            while (mm) { const int l = __builtin_ctzll(mm); mm &= mm - 1; L.tmp[l] = alloc_in_column(A, a, chunk, &status); }
            A.vr[k].app_cnt = a; A.vr[k].app_chunk = chunk;
        }
        __threadfence();
        WAVE_SYNC();
        if (act && status == 0) {
            const int32_t s_r = B.a_twin[j], s_n = L.tmp[lane];
            const double nw = newv[j];
            A.e[s_r].nbr = k; A.e[s_r].val = nw; A.e[s_r].twin = s_n;
            A.e[s_n].nbr = B.a_nbr[j]; A.e[s_n].val = nw; A.e[s_n].twin = s_r;
        }
        WAVE_SYNC();
        if (__ballot(status != 0) != 0ull) break;
    }
    if (__ballot(status != 0) != 0ull) { if (lane == 0) G.status = ST_POOL_OVERFLOW; WAVE_SYNC(); return true; }
    if (lane == 0) {
        if (m >= 1) A.e[B.a_twin[m - 1]].val = 0;   // :791-792
        G.n_draws = draws0 + ndraw;
    }
    WAVE_SYNC();
    return true;
}


// ---------------------------------------------------------------------------
// Batch kernel
// ---------------------------------------------------------------------------
// Two shapes of the workgroup: 1024 threads (4096 slots per round, ~156 KB LDS, one workgroup per CU) for a few large
// graphs; 256 threads (1024 slots, 39 KB and 128 VGPRs: four workgroups per CU) when a batch holds more graphs than the device has
// CUs -- small graphs give short rounds anyway and four of them hide each other's latency.
constexpr int PASSES = 4;     // (candidate, slot) pairs per thread: slots per round = 4 x threads

struct CRec { int32_t x, i, j; };
// contended (target, candidate) records a round may hold; more stop the round in front of the candidate.  The 16-slot shape gives
// half of the list to its 256 candidate records (its rounds average some 50 contended records)
constexpr int batch_ccap(int BC, int NTT) { return BC == 16 ? NTT / 4 : NTT / 2; }

template <int BC, int NTT>
struct BatchLdsT {
    CandT<BC> cand[4 * NTT / BC];
    union {
        struct {
            uint64_t mkey[NTT];   // PQ moves per round: one per thread, sorted in registers + LDS
            int32_t mval[NTT];
            int32_t hidx[NTT];
        };
        int32_t hcnt[4 * NTT];    // before the commit: counts of the target hash table (keys over pslot)
    };
    int32_t pslot[4 * NTT];   // slot of the entry position p of candidate i appends (commit phase)
    unsigned long long cmask[4 * NTT / BC];   // per candidate: which op numbers (mv - m) end in a PQ move -> order of the moves
    CRec cont[batch_ccap(BC, NTT)];       // contended (target, candidate) records per round
    CRec csorted[batch_ccap(BC, NTT)];
    int32_t scan[NTT / 64 + 8];
};

template <int BC, int NTT>
union ElimSharedT {
    BatchLdsT<BC, NTT> b;
    ElimLdsT<(NTT >= 1024 ? ECAP : ECAP_SMALL)> e;
    BigElimLdsT<(NTT >= 1024 ? 7168 : 1536)> g;
};
static_assert(sizeof(ElimSharedT<64, 1024>) == sizeof(BatchLdsT<64, 1024>) && sizeof(ElimSharedT<32, 1024>) == sizeof(BatchLdsT<32, 1024>) &&
              sizeof(ElimSharedT<16, 1024>) == sizeof(BatchLdsT<16, 1024>),
              "the single-vertex paths borrow the batch round's LDS");

// exclusive block scan over the workgroup's NWAVE waves; returns exclusive prefix, *total = sum
template <int NWAVE>
__device__ __noinline__ int block_excl_scan(int val, int* scratch, int* total) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int incl = val;
    for (int off = 1; off < 64; off <<= 1) { int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
    if (lane == 63) scratch[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < NWAVE; ++w) { int sw = scratch[w]; if (w < wave) base += sw; tot += sw; }
    __syncthreads();
    *total = tot;
    return base + incl - val;
}

// ordered block compaction helper: position of a flagged thread among flagged threads (thread order)
template <int NWAVE>
__device__ __forceinline__ int block_rank(bool flag, int* scratch, int* total) {
    return block_excl_scan<NWAVE>(flag ? 1 : 0, scratch, total);
}


// rewire stores of one push (preconditioner.cc:404-414)
__device__ __forceinline__ void rewire_store(const Arrays& A, int32_t s_r, int32_t s_n, int32_t nbr_j, int32_t k, double nw) {
    Slot a; a.val = nw; a.nbr = k; a.twin = s_n;
    Slot b; b.val = nw; b.nbr = nbr_j; b.twin = s_r;
    A.e[s_r] = a;     // one 16-byte store per slot
    A.e[s_n] = b;
}

// all pushes of candidate C into the column of its target at position j, in position order
template <class CT>
__device__ __forceinline__ void push_into_target(const Arrays& A, const CT& C, int32_t j, int32_t& a, int32_t& chunk, int32_t* status) {
    const int32_t x = C.e[j].nbr;
    if (A.o_v == OV_COARSEN) {
        if (j != C.koff) return;
        for (int32_t p = 0; p < C.m; ++p) {
            if (p == C.koff) continue;
            int32_t s_n = alloc_in_column(A, a, chunk, status);
            if (*status) return;
            rewire_store(A, C.e[p].twin, s_n, C.e[p].nbr, x, C.e[p].val);
        }
    } else {
        for (int32_t p = 0; p < C.m - 1; ++p) {
            if (C.ksel[p] != j) continue;
            int32_t s_n = alloc_in_column(A, a, chunk, status);
            if (*status) return;
            rewire_store(A, C.e[p].twin, s_n, C.e[p].nbr, x, C.e[p].val);
        }
    }
}

// slots for all pushes of candidate C into the column of its target at position j (position order)
template <class CT>
__device__ __forceinline__ void slots_into_target(const Arrays& A, const CT& C, int32_t j, int32_t& a, int32_t& chunk, int32_t* status, int32_t* pslot_row) {
    const bool co = A.o_v == OV_COARSEN;
    if (co && j != C.koff) return;
    const int32_t plast = co ? C.m : C.m - 1;
    for (int32_t p = 0; p < plast; ++p) {
        if (co ? (p == C.koff) : (C.ksel[p] != j)) continue;
        pslot_row[p] = alloc_in_column(A, a, chunk, status);
        if (*status) return;
    }
}

template <class CT>
__device__ __noinline__ void cand_order_index_call(const Arrays& A, CT& C) { cand_order_index(A, C); }

// rlap_core.h::cand_patch by one wave (32-slot candidates: one entry per lane of the lower half), followed by the sampling of
// the patched candidate.  d's entries live in registers while they are patched and ordered again: by id with a rank count
// (ids are distinct), by o_n with the half-wave std::sort restatement.  Returns false when d cannot be patched.
template <int ON, class CT>
__device__ __noinline__ bool wave_patch(const int32_t o_v, const uint64_t shuffle_seed, const double* __restrict__ rng, const int32_t rng_mode, CT* cand, int32_t d, int32_t vbase, int32_t* tmp_wave) {
    Arrays A;            // (by value, like cand_prepare_wide: what the sampling helpers read of the argument block; lives in registers)
    A.o_v = o_v; A.o_n = ON; A.shuffle_seed = shuffle_seed; A.rng = rng; A.rng_mode = rng_mode; A.vbase = vbase;
    static_assert(CT::CAP == 16 || CT::CAP == 32 || CT::CAP == 64, "one entry per lane");
    const int lane = lane_id();
    CT& C = cand[d];
    const int32_t m = C.m, nd = C.ndep, v = C.v;
    if (C.nkill > 0) return false;   // merged multi-edges (64-slot candidates): see rlap_core.h::cand_patch
    int32_t my_nbr = lane < m ? C.e[lane].nbr : -1;
    double my_val = lane < m ? C.e[lane].val : 0.0;
    int32_t my_twin = lane < m ? C.e[lane].twin : 0;
    bool ok = true, dup = false;
    for (int32_t q = 0; q < nd && ok; ++q) {
        const int32_t j = C.dep[q];
        const CT& J = cand[j];
        const int32_t mj = J.m;
        const int32_t jn = lane < mj ? J.e[lane].nbr : -2;
        const uint64_t pm = __ballot(jn == v);
        if (pm == 0ull) { ok = false; break; }
        const int32_t p = __builtin_ctzll(pm);
        if (p == mj - 1) { ok = false; break; }                                   // last neighbour (:420-432)
        const int32_t ks = lane < mj - 1 ? (int32_t)J.ksel[lane] : -1;
        if (__ballot(ks == p) != 0ull) { ok = false; break; }                     // sampled as a target (:394-399)
        const int32_t k = J.e[J.ksel[p]].nbr;
        const double newv = J.e[p].val;
        if (!(newv > 0)) { ok = false; break; }                                   // dead on arrival (rounding: f > 1), see cand_patch
        if (__ballot(my_nbr == k) != 0ull) { ok = false; dup = true; break; }     // multi-edge: single-vertex path
        const uint64_t qm = __ballot(my_nbr == J.v);
        if (qm == 0ull) { ok = false; break; }
        if (lane == __builtin_ctzll(qm)) { my_nbr = k; my_val = newv; my_twin = ~(j * CT::CAP + p); }
    }
    if (!ok) {
        if (lane == 0 && dup) atomicOr(&C.flags, CF_DUP);
        return false;
    }
    // order by id (:275): rank = smaller ids (distinct)
    int32_t rank = 0;
    for (int32_t q = 0; q < m; ++q) { const int32_t nq = __shfl(my_nbr, q); rank += (nq < my_nbr) ? 1 : 0; }
    {
        const int target = lane < m ? rank : lane;
        my_nbr = __builtin_amdgcn_ds_permute(target << 2, my_nbr);
        my_twin = __builtin_amdgcn_ds_permute(target << 2, my_twin);
        const long long bv = __double_as_longlong(my_val);
        const int lo = __builtin_amdgcn_ds_permute(target << 2, (int)(uint32_t)bv), hi = __builtin_amdgcn_ds_permute(target << 2, (int)(uint32_t)((unsigned long long)bv >> 32));
        my_val = __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
    }
    // order by o_n (:295-307) with std::sort semantics
    constexpr bool keyed = (ON == ON_RANDOM);
    double key = keyed ? keyed_order_dkey(keyed_order_base(A.shuffle_seed, v - vbase, 0), my_nbr - vbase) : my_val;
    int idx = lane & (CT::CAP - 1), pos = lane & (CT::CAP - 1);
    if constexpr (CT::CAP == 16) {
        // m <= 16: std::sort is an insertion sort, hence stable -- the position is the stable rank of the key (the entries sit in
        // lanes [0,m) in id order)
        int32_t r = 0;
        for (int32_t q = 0; q < m; ++q) {
            const double kq = __shfl(key, q);
            const bool before = (ON == ON_DESC) ? (kq > key) : (kq < key);
            r += (before || (kq == key && q < lane)) ? 1 : 0;
        }
        idx = lane; pos = r;
    } else if (CT::CAP == 32) {
        const bool want = lane < 32 && m > 1;
        const bool okg = (ON == ON_DESC) ? group_sort<true, 32>(key, idx, m, want, lane, tmp_wave, &pos) : group_sort<false, 32>(key, idx, m, want, lane, tmp_wave, &pos);
        if (__ballot(want && !okg) != 0ull) return false;   // depth limit of the introsort: leave it to the single-vertex path (conservative)
    } else if (m > 1) {
        const bool okg = (ON == ON_DESC) ? wave_sort64<true>(key, idx, m, lane, tmp_wave, &pos) : wave_sort64<false>(key, idx, m, lane, tmp_wave, &pos);
        if (!okg) return false;
    }
    {
        const int32_t nb = __shfl(my_nbr, idx), tw = __shfl(my_twin, idx);
        const double vv = __shfl(my_val, idx);
        WAVE_SYNC();
        if (lane < m) { Ent& E = C.e[pos]; E.nbr = nb; E.twin = tw; E.val = vv; E.aux = 0; }
    }
    WAVE_SYNC();
    // sampling of the patched candidate (P3 of the round, for this one candidate)
    if (lane == 0) cand_cumsum(A, C);
    WAVE_SYNC();
    if (lane < m - 1) cand_pick(A, C, lane);
    if (lane == 63) cand_recur(A, C);
    WAVE_SYNC();
    return true;
}

// ---------------------------------------------------------------------------
// Candidate preparation for 128-slot candidates (o_v = random on graphs whose columns run long: a column of 65..128 entries
// no longer ends the round).  ONE wave per candidate, two entries per lane: entry e = lane came in as (v0, n0, t0, a0),
// entry 64 + lane as (v1, ...); the caller has stored the raw (val, nbr) of every loaded slot at C.e[e].  Steps as in the
// 32/64-slot code: rank by id among the live entries (std::sort order where ids repeat), multi-edges folded (:278-293),
// o_n order with std::sort semantics (:295-307), permutation applied.  The sorts beyond 64 elements are the level-synchronous
// restatement over an index array (the keys stay in the record).  scr: WIDE_SCR_BYTES of LDS owned by this wave.
// ---------------------------------------------------------------------------
constexpr int WIDE_SCR_BYTES = 2048;

// Bitonic network over the 128 values a wave holds two per lane (element t*64 + lane in a[t]): ascending.  The exchanges
// with distance 64 stay inside the lane, the others are xor-shuffles.  Only the first KMAX elements (a power of two) matter
// to the caller, the rest is padding that compares last: the stages beyond KMAX are left out, and up to 64 the second register
// is left alone.  The second form sorts (key, source) pairs by key, then source -- a stable order.
template <int KMAX>
__device__ __forceinline__ void wave_bitonic_t(unsigned long long (&a)[2], int lane) {
#pragma unroll
    for (int kk = 2; kk <= KMAX; kk <<= 1) {
#pragma unroll
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            if (jj == 64) {
                if (a[1] < a[0]) { const unsigned long long t = a[0]; a[0] = a[1]; a[1] = t; }
            } else {
#pragma unroll
                for (int t = 0; t < (KMAX > 64 ? 2 : 1); ++t) {
                    const int e = t * 64 + lane;
                    const unsigned long long o = __shfl_xor(a[t], jj);
                    const bool keep_min = (((e & jj) == 0) == ((e & kk) == 0));
                    if (keep_min == (o < a[t])) a[t] = o;
                }
            }
        }
    }
}
template <int KMAX>
__device__ __forceinline__ void wave_bitonic_t(unsigned long long (&a)[2], int (&s)[2], int lane) {
#pragma unroll
    for (int kk = 2; kk <= KMAX; kk <<= 1) {
#pragma unroll
        for (int jj = kk >> 1; jj > 0; jj >>= 1) {
            if (jj == 64) {
                if (a[1] < a[0] || (a[1] == a[0] && s[1] < s[0])) { const unsigned long long t = a[0]; a[0] = a[1]; a[1] = t; const int u = s[0]; s[0] = s[1]; s[1] = u; }
            } else {
#pragma unroll
                for (int t = 0; t < (KMAX > 64 ? 2 : 1); ++t) {
                    const int e = t * 64 + lane;
                    const unsigned long long o = __shfl_xor(a[t], jj);
                    const int os = __shfl_xor(s[t], jj);
                    const bool keep_min = (((e & jj) == 0) == ((e & kk) == 0));
                    const bool other_less = o < a[t] || (o == a[t] && os < s[t]);
                    if (keep_min == other_less) { a[t] = o; s[t] = os; }
                }
            }
        }
    }
}
__device__ __forceinline__ void wave_bitonic128(unsigned long long (&a)[2], int lane, int count) {   // count: elements that matter (wave-uniform)
    if (count <= 16) wave_bitonic_t<16>(a, lane);
    else if (count <= 32) wave_bitonic_t<32>(a, lane);
    else if (count <= 64) wave_bitonic_t<64>(a, lane);
    else wave_bitonic_t<128>(a, lane);
}
__device__ __forceinline__ void wave_bitonic128(unsigned long long (&a)[2], int (&s)[2], int lane, int count) {
    if (count <= 16) wave_bitonic_t<16>(a, s, lane);
    else if (count <= 32) wave_bitonic_t<32>(a, s, lane);
    else if (count <= 64) wave_bitonic_t<64>(a, s, lane);
    else wave_bitonic_t<128>(a, s, lane);
}
struct WideIdLess { const Ent* e; __device__ bool operator()(uint16_t a, uint16_t b) const { return e[a].nbr < e[b].nbr; } };
struct WideAuxLess { const Ent* e; __device__ bool operator()(uint16_t a, uint16_t b) const { return e[a].aux < e[b].aux; } };
struct WideAuxGreater { const Ent* e; __device__ bool operator()(uint16_t a, uint16_t b) const { return e[a].aux > e[b].aux; } };

// (the three mode scalars by value, not `const Arrays&`: a reference to the kernel's argument block makes every call store a 200-byte
// copy of it to the stack -- 24 scratch stores per candidate in the round loop -- for three fields)
__device__ __noinline__ void cand_prepare_wide(const int32_t o_v, const int32_t o_n, const uint64_t shuffle_seed, CandT<128>& C, int32_t vbase, double v0, int32_t n0, int32_t t0, bool a0,
                                               double v1, int32_t n1, int32_t t1, bool a1, uint8_t* scr, const uint8_t* __restrict__ eqg) {
    ASSUME_LDS(&C); ASSUME_LDS(scr);
    Arrays A;            // what the callees below read of it (o_v, o_n); lives in registers
    A.o_v = o_v; A.o_n = o_n; A.shuffle_seed = shuffle_seed;
    const int lane = lane_id();
    const uint64_t lt = lanemask_lt(lane);
    const bool keyed = (A.o_n == ON_RANDOM || A.o_v == OV_COARSEN);
    const bool desc = (A.o_n == ON_DESC) && !keyed;
    uint16_t* const rec = reinterpret_cast<uint16_t*>(scr);
    uint16_t* const ulist = reinterpret_cast<uint16_t*>(scr + 256);
    uint16_t* const dlist = reinterpret_cast<uint16_t*>(scr + 520);
    uint32_t* const tab = reinterpret_cast<uint32_t*>(scr + 784);
    uint16_t* const tab2 = reinterpret_cast<uint16_t*>(scr + 1296);
    uint8_t* const posmap = scr + 1552;
    int32_t* const tmp64 = reinterpret_cast<int32_t*>(scr);   // wave_sort64's scratch (never live together with the arrays above)
    static_assert(1552 + 128 <= WIDE_SCR_BYTES && 256 * 4 <= WIDE_SCR_BYTES, "scratch layout");
    const int32_t ext = C.ext;   // slots loaded (dead ones included)
    const bool live0 = a0 && v0 > 0, live1 = a1 && v1 > 0;
    const uint64_t h0 = __ballot(live0), h1 = __ballot(live1);
    const int32_t nlive = popc64(h0) + popc64(h1);
    // ---- rank by id among the live entries (dead ones last); equal ids = multi-edges.  Key = (id, place in the traversal
    //      order): the network's order is the stable one, i.e. the insertion sort's ----
    // A column without appended entries whose CSR segment is still in order (in-place twin rewrites can break it: every slot,
    // live or dead, must lie strictly above its successor) is read in descending id: the rank is a count of the live entries behind.
    bool clean = false;
    if (C.acnt == 0 && ext <= 64) {   // (wave-uniform)
        const int32_t nxt = __shfl_down(n0, 1);
        clean = __ballot(a0 && (lane + 1 < ext) && !(n0 > nxt)) == 0ull;
    }
    int32_t r0, r1 = 0;
    bool anydup = false;
    if (clean) {
        r0 = popc64(h0 & ~((2ull << lane) - 1ull));
        if (lane == 63) r0 = 0;
        WAVE_SYNC();   // (the raw entries stored by the caller: not read on this path, but the stores below must come after them)
    } else {
    unsigned long long ik[2];
    ik[0] = ((unsigned long long)(live0 ? (uint32_t)n0 : 0x7FFFFFFFu) << 8) | (unsigned)lane;
    ik[1] = ((unsigned long long)(live1 ? (uint32_t)n1 : 0x7FFFFFFFu) << 8) | (unsigned)(64 + lane);
    wave_bitonic128(ik, lane, ext);   // (slots e >= ext hold nothing)
    {
        unsigned long long pv0 = __shfl_up(ik[0], 1), pv1 = __shfl_up(ik[1], 1);
        const unsigned long long edge = __shfl(ik[0], 63);
        if (lane == 0) { pv0 = ~0ull; pv1 = edge; }
        const bool du0 = (ik[0] >> 8) == (pv0 >> 8) && (ik[0] >> 8) != 0x7FFFFFFFull;
        const bool du1 = (ik[1] >> 8) == (pv1 >> 8) && (ik[1] >> 8) != 0x7FFFFFFFull;
        anydup = (__ballot(du0) | __ballot(du1)) != 0ull;
    }
    posmap[(int)(ik[0] & 0xFFull)] = (uint8_t)lane;
    posmap[(int)(ik[1] & 0xFFull)] = (uint8_t)(64 + lane);
    WAVE_SYNC();   // (also: the raw entries stored by the caller)
    r0 = posmap[lane]; r1 = posmap[64 + lane];
    WAVE_SYNC();
    }
    int32_t rk0 = r0, rk1 = r1;
    bool merge = false;
    if (anydup) {
        merge = true;
        if (nlive > 16) {   // (up to 16: insertion sort, the stable order above)
            // std::sort by id of the live entries in traversal order
            const int g0 = popc64(h0 & lt), g1 = popc64(h0) + popc64(h1 & lt);
            if (live0) rec[g0] = (uint16_t)lane;
            if (live1) rec[g1] = (uint16_t)(64 + lane);
            WAVE_SYNC();
            bool ok;
            if (nlive <= 64) {
                const int src = lane < nlive ? (int)rec[lane] : 0;
                WAVE_SYNC();
                double key = (double)C.e[src].nbr;
                int idx = src, pos = lane;
                ok = wave_sort64<false>(key, idx, nlive, lane, tmp64, &pos);
                WAVE_SYNC();
                if (ok && lane < nlive) posmap[idx] = (uint8_t)pos;
            } else {
                ok = wave_lvl_sort<uint16_t, WideIdLess, 2>(rec, nlive, WideIdLess{C.e}, ulist, dlist, tab, tab2, lane);
                if (ok) {
                    if (lane < nlive) posmap[rec[lane]] = (uint8_t)lane;
                    if (64 + lane < nlive) posmap[rec[64 + lane]] = (uint8_t)(64 + lane);
                }
            }
            WAVE_SYNC();
            if (!ok) {   // depth limit of the introsort: the single-vertex path takes this vertex
                if (lane == 0) atomicOr(&C.flags, CF_DUP);
                WAVE_SYNC();
                return;
            }
            if (live0) rk0 = posmap[lane];
            if (live1) rk1 = posmap[64 + lane];
        }
    }
    WAVE_SYNC();   // every read of the raw entries is done
    const uint64_t kb = keyed ? keyed_order_base(A.shuffle_seed, C.v - vbase, 0) : 0ull;
    if (live0) { Ent& E = C.e[rk0]; E.val = v0; E.nbr = n0; E.twin = t0; E.aux = keyed ? keyed_order_dkey(kb, n0 - vbase) : v0; }
    if (live1) { Ent& E = C.e[rk1]; E.val = v1; E.nbr = n1; E.twin = t1; E.aux = keyed ? keyed_order_dkey(kb, n1 - vbase) : v1; }
    WAVE_SYNC();
    int32_t m = nlive;
    if (merge) {
        // fold equal ids: the sum runs in sorted order (:284); the twins of the folded entries die at commit (:289)
        const bool c0 = lane < nlive, c1 = 64 + lane < nlive;
        const int32_t nb0 = c0 ? C.e[lane].nbr : -1, nb1 = c1 ? C.e[64 + lane].nbr : -1;
        const int32_t tw0 = c0 ? C.e[lane].twin : 0, tw1 = c1 ? C.e[64 + lane].twin : 0;
        double s0 = c0 ? C.e[lane].val : 0.0, s1 = c1 ? C.e[64 + lane].val : 0.0;
        const int32_t pv0 = (c0 && lane > 0) ? C.e[lane - 1].nbr : -2, pv1 = c1 ? C.e[63 + lane].nbr : -2;
        const bool hd0 = c0 && nb0 != pv0, hd1 = c1 && nb1 != pv1;
        const uint64_t hm0 = __ballot(hd0), hm1 = __ballot(hd1);
        m = popc64(hm0) + popc64(hm1);
        if (hd0) {
            const uint64_t above = (lane == 63) ? 0ull : (hm0 >> (lane + 1));
            const int nexthead = above ? (lane + 1 + __builtin_ctzll(above)) : (hm1 ? 64 + __builtin_ctzll(hm1) : nlive);
            for (int q = lane + 1; q < nexthead; ++q) s0 += C.e[q].val;
        }
        if (hd1) {
            const uint64_t above = (lane == 63) ? 0ull : (hm1 >> (lane + 1));
            const int nexthead = above ? (64 + lane + 1 + __builtin_ctzll(above)) : nlive;
            for (int q = 64 + lane + 1; q < nexthead; ++q) s1 += C.e[q].val;
        }
        const uint64_t nh0 = __ballot(c0 && !hd0), nh1 = __ballot(c1 && !hd1);
        const int32_t x0 = popc64(hm0 & lt), x1 = popc64(hm0) + popc64(hm1 & lt);
        const int32_t y0 = popc64(nh0 & lt), y1 = popc64(nh0) + popc64(nh1 & lt);
        WAVE_SYNC();
        if (hd0) { Ent& E = C.e[x0]; E.val = s0; E.nbr = nb0; E.twin = tw0; E.aux = keyed ? keyed_order_dkey(kb, nb0 - vbase) : s0; }
        else if (c0) C.e[m + y0].twin = tw0;
        WAVE_SYNC();   // (a lane's first entry may land where another lane's second one was read: all reads are above)
        if (hd1) { Ent& E = C.e[x1]; E.val = s1; E.nbr = nb1; E.twin = tw1; E.aux = keyed ? keyed_order_dkey(kb, nb1 - vbase) : s1; }
        else if (c1) C.e[m + y1].twin = tw1;
        if (lane == 0) { C.m = m; C.nkill = nlive - m; }
        WAVE_SYNC();
    } else if (lane == 0) C.m = nlive;
    if (m == 0) { WAVE_SYNC(); return; }
    // ---- o_n order: ksel[position] = source ----
    const bool c0 = lane < m, c1 = 64 + lane < m;
    const double k0 = c0 ? C.e[lane].aux : 0.0, k1 = c1 ? C.e[64 + lane].aux : 0.0;
    const double kfirst = C.e[0].aux;
    const bool alleq = (__ballot(c0 && k0 != kfirst) | __ballot(c1 && k1 != kfirst)) == 0ull;
    if (alleq) {   // std::sort of all-equal keys: identity up to 16, a fixed permutation above (k_eq_tables)
        if (c0) C.ksel[lane] = (m <= 16) ? (uint8_t)lane : eqg[(m - 17) * 128 + lane];
        if (c1) C.ksel[64 + lane] = eqg[(m - 17) * 128 + 64 + lane];
    } else {
        // stable rank by (key, position): a bitonic network over the keys' bit patterns (weights and keyed keys are positive
        // doubles: the patterns order like the values; complemented for the descending order); exact for m <= 16 (insertion
        // sort) and whenever no two keys are equal
        unsigned long long ok2[2];
        int os2[2] = {lane, 64 + lane};
        ok2[0] = c0 ? (desc ? ~(unsigned long long)__double_as_longlong(k0) : (unsigned long long)__double_as_longlong(k0)) : ~0ull;
        ok2[1] = c1 ? (desc ? ~(unsigned long long)__double_as_longlong(k1) : (unsigned long long)__double_as_longlong(k1)) : ~0ull;
        wave_bitonic128(ok2, os2, lane, m);
        bool anytie;
        {
            unsigned long long pv0 = __shfl_up(ok2[0], 1), pv1 = __shfl_up(ok2[1], 1);
            const unsigned long long edge = __shfl(ok2[0], 63);
            if (lane == 0) pv1 = edge;
            anytie = (__ballot(c0 && lane > 0 && ok2[0] == pv0) | __ballot(c1 && ok2[1] == pv1)) != 0ull;
        }
        if (m <= 16 || !anytie) {
            if (c0) C.ksel[lane] = (uint8_t)os2[0];
            if (c1) C.ksel[64 + lane] = (uint8_t)os2[1];
        } else {
            bool ok;
            if (m <= 64) {
                double key = k0;
                int idx = lane, pos = lane;
                ok = desc ? wave_sort64<true>(key, idx, m, lane, tmp64, &pos) : wave_sort64<false>(key, idx, m, lane, tmp64, &pos);
                if (ok && lane < m) C.ksel[pos] = (uint8_t)idx;
            } else {
                if (c0) rec[lane] = (uint16_t)lane;
                if (c1) rec[64 + lane] = (uint16_t)(64 + lane);
                WAVE_SYNC();
                ok = desc ? wave_lvl_sort<uint16_t, WideAuxGreater, 2>(rec, m, WideAuxGreater{C.e}, ulist, dlist, tab, tab2, lane)
                          : wave_lvl_sort<uint16_t, WideAuxLess, 2>(rec, m, WideAuxLess{C.e}, ulist, dlist, tab, tab2, lane);
                if (ok) { if (c0) C.ksel[lane] = (uint8_t)rec[lane]; if (c1) C.ksel[64 + lane] = (uint8_t)rec[64 + lane]; }
            }
            WAVE_SYNC();
            if (!ok && lane == 0) cand_order_index_call(A, C);   // depth limit: the sequential restatement
        }
    }
    WAVE_SYNC();
    // ---- apply the permutation ----
    double pv0 = 0, pv1 = 0; int32_t pn0 = 0, pn1 = 0, pt0 = 0, pt1 = 0;
    if (c0) { const Ent& Sx = C.e[C.ksel[lane]]; pv0 = Sx.val; pn0 = Sx.nbr; pt0 = Sx.twin; }
    if (c1) { const Ent& Sx = C.e[C.ksel[64 + lane]]; pv1 = Sx.val; pn1 = Sx.nbr; pt1 = Sx.twin; }
    WAVE_SYNC();
    if (c0) { Ent& E = C.e[lane]; E.val = pv0; E.nbr = pn0; E.twin = pt0; E.aux = 0; }
    if (c1) { Ent& E = C.e[64 + lane]; E.val = pv1; E.nbr = pn1; E.twin = pt1; E.aux = 0; }
    if (lane == 0) C.ndraw = (A.o_v == OV_COARSEN) ? 1 : (m > 1 ? m - 1 : 0);
    WAVE_SYNC();
}

__device__ __noinline__ void serial_eliminate_call(const Arrays& A, GraphDesc& G, const ElimScratch& S, int32_t v0, int64_t e1) {
    ColBuf Bf = S.colbuf(G.scr_base);
    int rc = serial_eliminate(A, G, Bf, G.scr_cap, v0, e1);
    if (rc) G.status = rc;
}

// Which positions of my candidate drew ME as their target (ksel[p] == j)?  A group of BC lanes = the positions of one candidate:
// lane p publishes ksel[p] bit by bit with ballots, lane j keeps the positions whose bits spell j.  Replaces the O(m) scan of
// ksel every (candidate, target) thread made in the replay and again when the slots are handed out.  Every lane of the wave calls.
template <int BC>
__device__ __forceinline__ uint64_t group_pick_mask(const uint8_t* ksel, int32_t m, bool cand_ok, int lane) {
    static_assert(BC == 32 || BC == 64, "one candidate per (half-)wave");
    constexpr int BITS = BC == 32 ? 5 : 6;
    const int gl = lane & (BC - 1), hb = lane & (64 - BC);
    const bool vp = cand_ok && gl < m - 1;       // position gl draws a target
    const int t = vp ? (int)ksel[gl] : 0;
    uint64_t mm = __ballot(vp);
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
        const uint64_t bb = __ballot(vp && ((t >> b) & 1));
        mm &= ((gl >> b) & 1) ? bb : ~bb;
    }
    return (mm >> hb) & (BC == 64 ? ~0ull : 0xFFFFFFFFull);
}

// Specialised on (o_v, o_n): the mode tests fold away, which keeps the round loop's code (executed once
// per round by every wave) small enough for the instruction cache.
template <int OV, int ON, int BC, int NTT>
__global__ __launch_bounds__(NTT, (NTT >= 1024 ? 1 : 4)) void k_eliminate_batch_t(Arrays A_in, GraphDesc* __restrict__ gd, ElimScratch S,
                                                           int32_t* __restrict__ batch_pos, const int32_t* __restrict__ in_flags,
                                                           const double* __restrict__ in_acc) {
    constexpr int NT = NTT;            // threads per workgroup
    // Workgroup barrier.  Debug (RLAP_DEBUG_JITTER=<n>, S.jitter): behind every barrier some waves -- a different set each time -- sleep
    // for n x 0.25 us, so that a value read behind a barrier while another wave already rewrites it (the push-id race of round 2) shows
    // in every run instead of once in some thousand.  Off: one scalar compare per barrier.
    uint32_t jit_ctr = 0;
#define BSYNC() do { __syncthreads(); if (S.jitter > 0) { ++jit_ctr; if (((((uint32_t)threadIdx.x >> 6) * 2654435761u + jit_ctr * 40503u) >> 7 & 3u) == 0u) \
        for (int _q = 0; _q < S.jitter; ++_q) __builtin_amdgcn_s_sleep(8); } } while (0)
    constexpr int NWAVE = NT / 64;
    constexpr int SLOTS = PASSES * NT; // candidates x slots per round
    constexpr int MCAP = NT;           // PQ moves per round
    constexpr int CCAP = batch_ccap(BC, NTT);   // contended records per round
    // 16 slots per candidate (degree order, while the columns at the head of the queue are short): 256 candidates per round, a
    // quarter-wave each.  A round whose FIRST candidate is longer ends the kernel, and the 32-slot kernel launched behind it on the
    // stream carries on from there (GraphDesc::resume).  m <= 16 throughout: std::sort is an insertion sort, no permutation tables.
    constexpr bool NARROW = (BC == 16);
    static_assert(!NARROW || (OV == OV_DEGREE && NTT == 1024), "the 16-slot shape exists for the degree order, 1024 threads");
    // a move's place in (candidate, op) order: candidate << SEQSH | op number (op numbers run to 2 m <= 2 BC); 15 bits in all
    constexpr int SEQSH = NARROW ? 6 : 8;
    static_assert(((SLOTS / BC - 1) << SEQSH | ((1 << SEQSH) - 1)) <= 0x7FFF && (BC > 32 || 2 * BC < (1 << SEQSH)), "(candidate, op) fits 15 bits");
    constexpr int HBITS = (SLOTS == 4096) ? 12 : (SLOTS == 2048) ? 11 : 10;   // log2(SLOTS): size of the target hash table
    static_assert((1 << HBITS) == SLOTS, "hash table = one place per slot");
    // BC slots per candidate: a group of BC lanes (half a wave or a whole wave) works on one candidate
    constexpr int BCAP = BC;
    constexpr int BATCH = SLOTS / BC;
    typedef CandT<BC> Cand;
    typedef BatchLdsT<BC, NTT> BatchLds;
    constexpr bool MERGE = (BC >= 64 && OV == OV_RANDOM);           // multi-edges merged inside the candidate (rlap_core.h::cand_merges_multi_edges)
    // candidates adjacent to earlier ones of the round are patched in LDS (rlap_core.h::cand_patch).  Measured: pays for the degree
    // order (C3 369 -> 274 ms); with o_v = random (64-slot candidates; wave_patch handles them too) the rounds of config 5 get 6.5 %
    // fewer and no faster, and the coarsening order fills its rounds without it -- so only the degree order uses it.
    constexpr bool PATCH = (OV == OV_DEGREE);
    // the replay (P4) sees only the (candidate, target) pairs rlap_core.h::cand_touches passes: about half of a degree-order
    // candidate's pairs name a target nobody picked, which keeps its key and gets nothing appended.  The PQ orders (16 and 32 slots)
    // take the rule; o_v = random (64 and 128 slots) has no keys to replay and finds its picks with ballots: it keeps every pair.
    constexpr bool SKIP = (BC <= 32);
    constexpr int GSH = BC >= 64 ? 0 : 64 - BC;                   // lane & GSH = first lane of my group
    constexpr uint64_t GMASK = BC >= 64 ? ~0ull : ((1ull << (BC & 63)) - 1ull);   // a group's part of a 64-bit ballot
    Arrays A = A_in;
    A.o_v = OV;
    A.o_n = ON;
    A.shuffle_seed = A_in.shuffle_seed + (uint64_t)blockIdx.x;   // graph g of a batch: seed + g, ids local to the graph (rlap_core.h)
    A.vbase = gd[blockIdx.x].vbase;
    __shared__ ElimSharedT<BC, NTT> sh;
    __shared__ GraphDesc G;
    __shared__ int32_t s_help[3];      // hand-over between the eliminating wave and its helper (single_helper); [2]: the helper gave up waiting
    __shared__ int32_t s_nc, s_pmax, s_p, s_ncont, s_nmoves, s_status, s_nhigh, s_nlow, s_pool_cur, s_pool_end, s_anydep, s_npatched;
    // chunk directory of the bucket the pops come from, kept in LDS between rounds: the prediction's stack window then starts with
    // the entries themselves instead of a dependent look-up of their chunk base (one global round trip less per round).
    // s_dirb = that bucket (global index), -1 none; refreshed when the bucket changes, a push allocates a chunk for it (push phase,
    // same thread) or the single-vertex path has pushed (it allocates through bs_ensure)
    __shared__ int32_t s_dirb;
    __shared__ int32_t s_dir[BDIR];
    constexpr int32_t POOL_GRAB = NT >= 1024 ? POOL_GRAB_BIG : POOL_GRAB_SMALL;   // slots reserved at a time for the round's appends
    // std::sort's permutation of n = 17..BC all-equal keys and its inverse (final position of the entry with id-rank r):
    // in LDS for the 1024-thread shape; the 256-thread shape reads the handle's tables (k_eq_tables) through the L1,
    // which leaves its LDS at 39 KB -- four workgroups per CU
    constexpr bool EQG = NTT < 1024 || BC == 128 || NARROW;   // (16 slots: no tables at all)
    constexpr int EC1 = NTT >= 1024 ? ECAP : ECAP_SMALL;   // single-vertex path in LDS up to this extent
    __shared__ uint8_t s_eqperm[EQG ? 1 : BC - 16][EQG ? 1 : BC];
    __shared__ uint8_t s_eqinv[EQG ? 1 : BC - 16][EQG ? 1 : BC];
    const uint8_t* __restrict__ eqg = S.eqtab + (BC == 64 ? 0 : (BC == 128 ? EQTAB_OFF128 : EQTAB_OFF32));
    BatchLds& L = sh.b;
    const int g = blockIdx.x;
    const int tid = threadIdx.x;
    if (S.poison >= 0) {   // debug: LDS starts as this byte, not as what the previous workgroup on this CU left behind
        uint32_t* const w = reinterpret_cast<uint32_t*>(&sh);
        const uint32_t pat = 0x01010101u * (uint32_t)(S.poison & 0xFF);
        for (size_t q = tid; q < sizeof(sh) / 4; q += NT) w[q] = pat;
        BSYNC();
    }
    if (tid == 0) {
        G = gd[g]; s_nc = 0; s_pmax = BATCH + 1; s_p = BATCH + 1; s_ncont = 0; s_nmoves = 0; s_pool_cur = 0; s_pool_end = 0; s_anydep = 0; s_npatched = 0;
        s_help[0] = 0; s_help[1] = 0; s_help[2] = 0; s_dirb = -1;
        if (G.resume) { s_pool_cur = G.pool_cur; s_pool_end = G.pool_end; }   // what the launch before this one had reserved and not used
        // the input checks of the setup kernels are read here, not on the host (no mid-call synchronisation): bad input -> nothing is eliminated
        int32_t bad = 0;
        if (in_flags[FLAG_RANGE]) bad = ST_INDEX_RANGE;
        else if (in_flags[FLAG_CROSS] || in_flags[FLAG_PERM]) bad = ST_BAD_ARG;
        else if (in_acc[2] != 0.0 || !(in_acc[0] <= 1e-24 * in_acc[1])) bad = ST_NOT_SYMMETRIC;   // isApprox(A^T), factorizers.cc:19-22
        s_status = bad;
    }
    if constexpr (!EQG) {
        for (int base = 0; base < BC - 16; base += BATCH) {   // the candidate records serve as scratch: BATCH lengths at a time
            const int row = base + tid;
            if (tid < BATCH && row < BC - 16) {
                Cand& C = L.cand[tid];
                const int nn = 17 + row;
                for (int q = 0; q < nn; ++q) { C.e[q].aux = 1.0; C.ksel[q] = (uint8_t)q; }
                C.m = nn;
                Arrays A3 = A;
                cand_order_index_call(A3, C);   // all keys equal: asc and desc compare alike
                for (int q = 0; q < BC; ++q) s_eqperm[row][q] = q < nn ? C.ksel[q] : (uint8_t)q;
                for (int q = 0; q < BC; ++q) s_eqinv[row][s_eqperm[row][q]] = (uint8_t)q;
            }
        }
    }
    BSYNC();
    const int32_t n = G.n;
    const bool use_pq = A.o_v != OV_RANDOM;
    int64_t nelim = G.t < (int64_t)(n - 1) ? G.t : (int64_t)(n - 1);
    if (nelim < 0 || s_status != 0) nelim = 0;
    int64_t done = 0;
    int32_t rounds = 0, singles = 0;
    if (G.resume) {
        // a later segment of a depths call: every round ends in a state the next round starts from (the PQ cursors move only for
        // committed pops and empty buckets, uncommitted candidates leave nothing behind but batch_pos, cleared in the epilogue), so
        // the loop picks up at the previous launch's n_elim.  The pool reservation comes along in the descriptor (pool_cur, pool_end);
        // the rest of the LDS-only state starts afresh: the chunk directory cache, and `pending_long` -- a long column
        // that cut the last round is popped first again and goes to the single-vertex path as first_is_big.
        done = G.n_elim; rounds = G.pad0; singles = G.pad1;
        if (G.status != 0 || nelim < done) nelim = done;   // an earlier segment failed (or the depth did not grow): nothing to do
        if (NARROW && G.narrow) nelim = done;              // handed over in an earlier segment: the 32-slot kernel behind this one goes on
    }
    const int32_t rounds_in = rounds, singles_in = singles;
    bool handover = false;     // 16-slot shape: the next vertex's column is longer than 16 slots
    bool pending_long = false;   // o_v = random: the last round was cut by a long column, which is therefore the next vertex
    long long t_prev = 0;
    __shared__ long long s_prof[40];   // diagnostic build only (S.prof != nullptr)
#define PHASE_STAMP(k) do { if (S.prof && tid == 0 && g == 0) { long long _t = wall_clock64(); s_prof[k] += _t - t_prev; t_prev = _t; } } while (0)
    long long clk0 = 0, wall0 = 0;
    if (S.prof && tid == 0 && g == 0) { for (int q = 0; q < 40; ++q) s_prof[q] = 0; t_prev = wall_clock64(); clk0 = clock64(); wall0 = t_prev; }

    while (done < nelim) {
        // per-round opaque copy of the thread id: keeps the compiler from hoisting the (cheap) per-pass index
        // and LDS-address arithmetic out of the round loop, where it would stay live across every barrier
        // and get spilled to scratch memory
        int tid_round = threadIdx.x;
        asm volatile("" : "+v"(tid_round));
        const int tid = tid_round;
        const int lane = tid & 63;
        // thread <-> (candidate, position) in the replay and commit phases.  64-slot candidates (o_v = random): a wave is one candidate,
        // so that its lanes can match positions and targets with ballots (group_pick_mask; config 5: 19.9 -> 18.6 ms).  The others keep
        // the interleaved layout (8 or 32 lanes per candidate and pass) and scan ksel: with 32-slot candidates the grouped layout keeps all
        // four passes busy where the interleaved one skips the last two for short candidates (measured: C3 285 -> 305 ms with it)
        constexpr bool GROUPED = (BC == 64);
        auto PI = [&](int k) -> int32_t { return GROUPED ? (k * NT + tid) / BCAP : tid / (NT / BATCH); };
        auto PJ = [&](int k) -> int32_t { return GROUPED ? (k * NT + tid) % BCAP : k * (NT / BATCH) + tid % (NT / BATCH); };
        if (OV == OV_RANDOM && pending_long) {
            // the vertex that cut the previous round goes straight to the single-vertex path: no round is set up around it
            pending_long = false;
            ++singles;
            const int32_t v0 = G.vbase + (int32_t)A.perm[G.vbase + n - (done + 1)];
            if (tid < 64) {
                Arrays A2 = A;
                ElimScratch S2 = S;
                int32_t cp0 = A2.colptr[v0], cp1 = A2.colptr[v0 + 1];
                int32_t acnt = A2.vr[v0].app_cnt, abase = A2.vr[v0].app_chunk;
                if ((cp1 - cp0) + acnt > EC1) {
                    ColBuf Bf = S2.colbuf(G.scr_base);
                    const bool handled = wave_eliminate_big(A2, G, sh.g, Bf, G.scr_cap, v0, cp0, cp1, acnt, abase, s_help);
                    if (!handled && lane == 0) {   // (a column the long-column path took has told the helper itself)
                        // no help wanted: said BEFORE the one-lane elimination, which may last longer than the helper's wait
                        __hip_atomic_store(&s_help[0], 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        serial_eliminate_call(A2, G, S2, v0, done + 1);
                    }
                } else {
                    wave_eliminate(A2, G, sh.e, v0, done + 1, cp0, cp1, acnt, abase, (S.prof && g == 0) ? &s_prof[24] : nullptr, s_help);
                }
            } else if (tid < 128) {
                single_helper(sh.e, sh.g.c.newv, s_help);
            }
            BSYNC();
            if (G.status != 0 || s_help[2] != 0) { if (tid == 0) s_status = G.status ? G.status : ST_INTERNAL; BSYNC(); break; }
            done += 1;
            PHASE_STAMP(5);
            continue;
        }
        ++rounds;
        // (16-slot shape: fewer candidates than the records hold -- the move list ends a round at about 160 committed, and what is
        // prepared, sampled and replayed beyond that is thrown away; the target hash table also fills to 0.6 with all 256)
        const int32_t bcap = NARROW ? (S.narrow_batch < BATCH ? S.narrow_batch : BATCH) : BATCH;
        const int32_t Bcur = (int32_t)((nelim - done) < (int64_t)bcap ? (nelim - done) : (int64_t)bcap);
        // ================= P0: predict the next pops =================
        // (the round counters were reset before the barrier that ended the previous round)
        int32_t b = 0;
        if (use_pq) {
            while (true) {
                b = G.bucket_base + G.minlist;
                const int32_t cnt = A.bs_cnt[b];
                int32_t oc0 = A.ocur[b];
                const int32_t oe = A.oend[b];
                if (s_dirb != b) {   // (workgroup-uniform: s_dirb changes only in front of a barrier)
                    if (tid < BDIR) s_dir[tid] = A.bs_dir[(int64_t)b * BDIR + tid];
                    BSYNC();
                    if (tid == 0) s_dirb = b;
                }
                // moved members, newest first, then the never-moved members in descending id.  The window of
                // the stack that reaches its bottom is read together with the first window of the never-moved
                // members (both load chains in flight at once, one block scan for the two).
                int32_t top = cnt;   // entries [0,top) not yet scanned
                while (s_nc < Bcur && (top > 0 || oc0 < oe)) {
                    const int32_t a = top - 1 - tid;
                    bool vs = false, vo = false;
                    int32_t v_s = -1, v_o = -1;
                    if (a >= 0) {
                        const int cdir = bs_chunk_of(a);
                        const int32_t sl = s_dir[cdir] + (a - bs_chunk_start(cdir));
                        v_s = A.bs_v[sl];
                        vs = (A.vr[v_s].pqpos == A.bs_id[sl]);
                    }
                    const bool last_stack = top <= NT;
                    const int32_t oc = oc0 + tid;
                    if (last_stack && oc < oe) { v_o = A.orig_order[oc]; vo = (A.vr[v_o].pqpos == -1); }
                    int tot;
                    const int r = block_excl_scan<NWAVE>((vs ? 1 : 0) | (vo ? (1 << 16) : 0), L.scan, &tot);
                    const int rs = r & 0xFFFF, ro = r >> 16, ts = tot & 0xFFFF, to = tot >> 16;
                    const int base = s_nc;
                    BSYNC();
                    if (vs && base + rs < Bcur) { L.cand[base + rs].v = v_s; L.cand[base + rs].src = a; }
                    if (vo && base + ts + ro < Bcur) { L.cand[base + ts + ro].v = v_o; L.cand[base + ts + ro].src = ~oc; }
                    if (tid == 0) s_nc = (base + ts + to < Bcur) ? base + ts + to : Bcur;
                    BSYNC();
                    top = top > NT ? top - NT : 0;
                    if (last_stack) oc0 += NT;
                }
                if (s_nc > 0) break;
                BSYNC();
                if (tid == 0) {
                    A.bs_cnt[b] = 0; A.ocur[b] = oe;
                    G.minlist += 1;
                    if (G.minlist > 2 * n) s_status = ST_INTERNAL;
                }
                BSYNC();
                if (s_status) break;
            }
            if (s_status) break;
        } else {
            if (tid < Bcur) { L.cand[tid].v = G.vbase + (int32_t)A.perm[G.vbase + n - (done + tid + 1)]; L.cand[tid].src = 0; }
            if (tid == 0) s_nc = Bcur;
            BSYNC();
        }
        const int32_t nc = s_nc;
        PHASE_STAMP(0);

        // ================= P1: prepare =================
        // (a) per candidate: column extent + chunk bases; (b) per slot: the loads; (c) per candidate: filter + sorts
        if (tid < nc) {
            int32_t v = L.cand[tid].v, src = L.cand[tid].src;
            cand_meta(A, v, L.cand[tid]);
            L.cand[tid].src = src;
            batch_pos[v] = tid;
            if (L.cand[tid].flags & CF_BIG) atomicMin(&s_pmax, tid);   // a long column cuts the round: nothing is loaded behind it
        }
        BSYNC();
        const bool first_is_big = (L.cand[0].flags & CF_BIG) != 0;   // goes to the single-vertex path: skip this round's prepare
        if constexpr (NARROW) {
            if (first_is_big) {
                // hand over: the queue is as the prediction found it (nothing popped), the marks of this round's candidates are taken
                // back, and the round is not counted -- the 32-slot kernel predicts it again
                if (tid < nc) batch_pos[L.cand[tid].v] = -1;
                --rounds;
                handover = true;
                break;
            }
        }
        if (!first_is_big) {
            // BATCH*BCAP = 4*NT slots: issue every load before the first LDS store
            static_assert(BATCH * BCAP == PASSES * NT && (BC == 16 || BC == 32 || BC == 64 || BC == 128), "slot loops are unrolled for PASSES passes");
            // slot of pass k -> (candidate, entry).  128-slot candidates: a wave owns a candidate, its entries lane and 64 + lane are
            // the wave's passes 2c and 2c+1 (everything candidate-local stays inside one wave)
            auto SI = [&](int k) -> int32_t { return BC == 128 ? ((k >> 1) * NWAVE + (tid >> 6)) : (k * NT + tid) / BCAP; };
            auto SE = [&](int k) -> int32_t { return BC == 128 ? (((k & 1) << 6) + (tid & 63)) : (k * NT + tid) % BCAP; };
            double lv[PASSES]; int32_t ln[PASSES], lt[PASSES]; bool la[PASSES];
            const int32_t cut0 = (OV == OV_RANDOM) ? s_pmax : nc;   // o_v = random: the first long column (most rounds have one) is known already
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int32_t i = SI(k), e = SE(k);
                la[k] = (i < nc) && (OV != OV_RANDOM || i < cut0) && (e < L.cand[i].ext);
                lv[k] = 0; ln[k] = 0; lt[k] = 0;
                if (la[k]) {
                    int32_t sl = cand_slot(L.cand[i], e);
                    const Slot g = A.e[sl]; lv[k] = g.val; ln[k] = g.nbr; lt[k] = g.twin;
                }
            }
            // dependence: is a live neighbour an earlier candidate of this round?  Looked up now (only the ids are needed), so
            // that the cut is known before the sorts: nothing more is prepared for the candidates behind it.
            int32_t bpk[PASSES];
#pragma unroll
            for (int k = 0; k < PASSES; ++k) { bpk[k] = -1; if (la[k] && lv[k] > 0) bpk[k] = batch_pos[ln[k]]; }
            // Shortcut for the common column: no appended entries, CSR segment still sorted, all live
            // weights equal, weight order.  Read backwards it is in descending id, so the id rank is a
            // popcount of the live mask; std::sort of all-equal keys is the identity up to 16 entries and a
            // fixed permutation above: every entry goes straight to its final position.
            const bool keyed = (A.o_n == ON_RANDOM || A.o_v == OV_COARSEN);
            bool ready[PASSES];
#pragma unroll
            for (int k = 0; k < PASSES; ++k) ready[k] = false;
            if constexpr (BC <= 64) {
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int32_t idx = k * NT + tid;
                const int32_t i = idx / BCAP, e = idx % BCAP;
                const int hb = lane & GSH;
                const bool live = la[k] && lv[k] > 0;
                const uint64_t half = (__ballot(live) >> hb) & GMASK;
                const int32_t nxt = __shfl_down(ln[k], 1);
                const bool cand_ok = (i < nc) && (OV != OV_RANDOM || i < cut0) && !(L.cand[i].flags & CF_BIG);
                const int32_t ext = cand_ok ? L.cand[i].ext : 0;
                const bool unsorted = la[k] && (e + 1 < ext) && !(ln[k] > nxt);
                const uint64_t hbad = (__ballot(unsorted) >> hb) & GMASK;
                const int f = half ? __builtin_ctzll(half) : 0;
                const double w0 = __shfl(lv[k], hb + f);
                const uint64_t hdw = (__ballot(live && lv[k] != w0) >> hb) & GMASK;
                ready[k] = cand_ok && !keyed && L.cand[i].acnt == 0 && hbad == 0 && hdw == 0;
                if (ready[k]) {
                    Cand& C = L.cand[i];
                    const int32_t m = __popcll(half);
                    if (live) {
                        const int32_t r = __popcll(half & ~((2ull << e) - 1ull));
                        const int32_t pos = (NARROW || m <= 16) ? r : (int32_t)(EQG ? eqg[(BC - 16) * BC + (m - 17) * BC + r] : s_eqinv[EQG ? 0 : m - 17][EQG ? 0 : r]);
                        Ent& E = C.e[pos];
                        E.val = lv[k]; E.nbr = ln[k]; E.twin = lt[k]; E.aux = 0;
                    }
                    if (e == 0) {
                        C.m = m;
                        C.ndraw = m > 1 ? m - 1 : 0;
                        C.flags |= CF_READY;
                    }
                    la[k] = false;   // nothing left to do for this slot
                }
            }
            }
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                if (la[k]) {
                    Ent& E = L.cand[SI(k)].e[SE(k)];
                    E.val = lv[k]; E.nbr = ln[k];
                }
            }
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int32_t i = SI(k);
                if (bpk[k] >= 0 && bpk[k] < i) {
                    if (PATCH) {
                        // adjacent to an earlier candidate of the round: remembered, patched after that one is sampled (wave_patch)
                        const int32_t q = atomicAdd(&L.cand[i].ndep, 1);
                        if (q < DEPMAX) L.cand[i].dep[q] = (uint8_t)bpk[k]; else atomicMin(&s_pmax, i);
                        s_anydep = 1;
                    } else atomicMin(&s_pmax, i);
                }
            }
            if (tid < nc && (L.cand[tid].flags & CF_BIG)) atomicMin(&s_pmax, tid);
            BSYNC();
            const int32_t ncp = s_pmax < nc ? s_pmax : nc;   // candidates [ncp, nc) are behind the cut
#pragma unroll
            for (int k = 0; k < PASSES; ++k) if (SI(k) >= ncp) { la[k] = false; ready[k] = false; }
            PHASE_STAMP(9);
            if constexpr (BC == 128) {
                // 128-slot candidates: the wave prepares its (at most two) candidates one after the other (cand_prepare_wide);
                // sort scratch in the hash / slot tables, which are idle until the barrier that ends P1
                uint8_t* const wscr = reinterpret_cast<uint8_t*>(L.hcnt) + (size_t)(tid >> 6) * WIDE_SCR_BYTES;
                static_assert((size_t)NWAVE * WIDE_SCR_BYTES <= sizeof(int32_t) * 8 * (size_t)NT, "scratch of the waves fits hcnt + pslot");
#pragma unroll
                for (int cc = 0; cc < PASSES / 2; ++cc) {
                    const int32_t i = cc * NWAVE + (tid >> 6);
                    if (i < ncp && !(L.cand[i].flags & CF_BIG)) {   // (wave-uniform)
                        cand_prepare_wide(A.o_v, A.o_n, A.shuffle_seed, L.cand[i], G.vbase, lv[2 * cc], ln[2 * cc], lt[2 * cc], la[2 * cc], lv[2 * cc + 1], ln[2 * cc + 1], lt[2 * cc + 1], la[2 * cc + 1], wscr, eqg);
                    }
                }
            } else {
            // rank of every live entry among its column's live entries by id: with distinct ids the
            // sorted order is unique, so no std::sort emulation is needed (equal ids -> single-vertex path).
            // One half-wave = one candidate.  A column without appended entries whose CSR segment is still
            // sorted is read in descending id, so its rank is a popcount of the live mask; others loop.
            int32_t rk[PASSES];
            bool merge_k[PASSES];
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                rk[k] = -1; merge_k[k] = false;
                if (__ballot(la[k]) == 0ull) continue;   // wave-uniform: nothing left in this pass for this wave
                const int32_t idx = k * NT + tid;
                const int32_t i = idx / BCAP, e = idx % BCAP;
                const bool live = la[k] && lv[k] > 0;
                const uint64_t half = (__ballot(live) >> (lane & GSH)) & GMASK;
                // in-place twin rewrites (:404-406) can leave a CSR segment unsorted: the shortcut needs
                // every slot (live or dead) strictly above its successor
                const int32_t nxt = __shfl_down(ln[k], 1);
                const bool unsorted = la[k] && (i < ncp) && (e + 1 < L.cand[i].ext) && !(ln[k] > nxt);
                const uint64_t hbad = (__ballot(unsorted) >> (lane & GSH)) & GMASK;
                rk[k] = -1;
                if (!ready[k] && i < ncp && L.cand[i].ext > 0) {
                    Cand& C = L.cand[i];
                    if (C.acnt == 0 && hbad == 0) {
                        if (live) rk[k] = __popcll(half & ~((2ull << e) - 1ull));
                        if (e == 0) C.m = __popcll(half);
                    } else if (!MERGE) {
                        // columns with appended entries (or an unsorted CSR segment): rank by id with a bitonic network over the
                        // half-wave's registers -- (id, lane) pairs, dead entries last; equal ids = multi-edge -> single-vertex path
                        uint32_t skey = live ? (uint32_t)ln[k] : 0x7FFFFFFFu;
                        int ssrc = e;
#pragma unroll
                        for (int kk = 2; kk <= BC; kk <<= 1) {
#pragma unroll
                            for (int jj = kk >> 1; jj > 0; jj >>= 1) {
                                const uint32_t okey = (uint32_t)__shfl_xor((int)skey, jj);
                                const int osrc = __shfl_xor(ssrc, jj);
                                const bool keep_min = (((e & jj) == 0) == ((e & kk) == 0));
                                const bool other_less = okey < skey || (okey == skey && osrc < ssrc);
                                if (keep_min == other_less) { skey = okey; ssrc = osrc; }
                            }
                        }
                        // lane p now holds the p-th pair: tell the source lane its rank (forward permute), look for equal neighbours
                        const uint32_t pkey = (uint32_t)__shfl_up((int)skey, 1);
                        const bool dupp = e > 0 && skey == pkey && skey != 0x7FFFFFFFu;
                        const int myrank = __builtin_amdgcn_ds_permute(((lane & GSH) + ssrc) << 2, e);
                        if (__ballot(dupp) >> (lane & GSH) & GMASK) { if (e == 0) atomicOr(&C.flags, CF_DUP); }
                        if (live) rk[k] = myrank;
                        if (e == 0) C.m = __popcll(half);
                    } else {
                        // one wave = this candidate.  Multi-edges are merged here (no PQ to replay in this mode): the
                        // position std::sort by id gives every live entry (stable rank up to 16 entries, the
                        // introsort restatement above), then merge_k[] below folds equal ids.
                        const int32_t ext = C.ext, me = ln[k];
                        int32_t r = 0, eqb = 0;
                        bool dup = false;
                        if (live) {
                            for (int32_t q = 0; q < ext; ++q) {
                                bool lq = C.e[q].val > 0;
                                int32_t nq = C.e[q].nbr;
                                r += (lq && nq < me) ? 1 : 0;
                                eqb += (lq && nq == me && q < e) ? 1 : 0;
                                dup |= (lq && nq == me && q != e);
                            }
                        }
                        const int32_t nlive = __popcll(half);
                        const bool anydup = __ballot(live && dup) != 0ull;
                        if (!anydup) {
                            if (live) rk[k] = r;
                        } else if (nlive <= 16) {
                            if (live) rk[k] = r + eqb;
                            merge_k[k] = true;
                        } else {
                            int32_t* tmp = L.pslot + (tid >> 6) * 256;   // pslot is not live before the commit
                            if (live) tmp[144 + __popcll(half & lanemask_lt(lane))] = lane;   // gather order = traversal order
                            WAVE_SYNC();
                            const int src = lane < nlive ? tmp[144 + lane] : 0;
                            double key = (double)__shfl(me, src);
                            int idx = src, pos = lane;
                            const WS64 wr = wave_sort64_call<false>(key, idx, nlive, lane, tmp);
                            key = wr.key; idx = wr.idx; pos = wr.pos;
                            const bool ok = wr.ok != 0;
                            WAVE_SYNC();
                            if (lane < nlive) tmp[144 + idx] = pos;
                            WAVE_SYNC();
                            if (ok) { if (live) rk[k] = tmp[144 + lane]; merge_k[k] = true; }
                            else if (lane == 0) atomicOr(&C.flags, CF_DUP);   // depth limit hit: single-vertex path
                            WAVE_SYNC();
                        }
                        if (lane == 0) C.m = nlive;
                    }
                }
            }
            WAVE_SYNC();   // candidate-local: producer and consumer are the same (half-)wave
            PHASE_STAMP(12);
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                if (__ballot(rk[k] >= 0) == 0ull) continue;
                if (rk[k] >= 0) {
                    const int32_t idx = k * NT + tid;
                    Cand& C = L.cand[idx / BCAP];
                    Ent& E = C.e[rk[k]];
                    E.val = lv[k]; E.nbr = ln[k]; E.twin = lt[k];
                    E.aux = keyed ? keyed_order_dkey(keyed_order_base(A.shuffle_seed, C.v - G.vbase, 0), ln[k] - G.vbase) : lv[k];
                }
            }
            if (MERGE) {
#pragma unroll
                for (int k = 0; k < PASSES; ++k) {
                    if (!merge_k[k]) continue;   // wave-uniform
                    WAVE_SYNC();
                    Cand& C = L.cand[k * NWAVE + (tid >> 6)];
                    const int32_t nl = C.m;
                    const bool act = lane < nl;
                    const int32_t nb = act ? C.e[lane].nbr : -1;
                    const int32_t tw = act ? C.e[lane].twin : 0;
                    double val = act ? C.e[lane].val : 0.0;
                    const int32_t nbprev = __shfl_up(nb, 1);
                    const bool head = act && (lane == 0 || nb != nbprev);
                    const uint64_t hm = __ballot(head), lt = lanemask_lt(lane);
                    const int32_t m = __popcll(hm);
                    if (head) {   // the sum runs in sorted order (:284)
                        const uint64_t above = (lane == 63) ? 0ull : (hm >> (lane + 1));
                        const int nexthead = above ? (lane + 1 + __builtin_ctzll(above)) : nl;
                        for (int q = lane + 1; q < nexthead; ++q) val += C.e[q].val;
                    }
                    const int32_t x = __popcll(hm & lt);
                    const int32_t y = __popcll(__ballot(act && !head) & lt);
                    WAVE_SYNC();
                    if (head) {
                        Ent& E = C.e[x];
                        E.val = val; E.nbr = nb; E.twin = tw;
                        E.aux = keyed ? keyed_order_dkey(keyed_order_base(A.shuffle_seed, C.v - G.vbase, 0), nb - G.vbase) : val;
                    } else if (act) {
                        C.e[m + y].twin = tw;   // dies at commit (:289)
                    }
                    if (lane == 0) { C.m = m; C.nkill = nl - m; }
                }
            }
            PHASE_STAMP(15);
            PHASE_STAMP(18);
            WAVE_SYNC();   // candidate-local: producer and consumer are the same (half-)wave
            PHASE_STAMP(16);
            // o_n order with std::sort semantics under ties.  All-equal keys (unit weights): identity for
            // m <= 16, a precomputed permutation above.  Otherwise a stable rank is exact for m <= 16
            // (pure insertion sort) and whenever the keys are distinct; the rest is emulated by one thread.
            const bool desc = (A.o_n == ON_DESC) && !keyed;
            int32_t r2[PASSES];
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                r2[k] = -1;
                const int32_t idx = k * NT + tid;
                const int32_t i = idx / BCAP, j = idx % BCAP;
                const bool valid = (i < ncp) && !(L.cand[i].flags & (CF_BIG | CF_DUP | CF_READY)) && (j < L.cand[i].m);
                if (__ballot(valid) == 0ull) continue;
                double kme = 0, k0 = 0;
                if (valid) { kme = L.cand[i].e[j].aux; k0 = L.cand[i].e[0].aux; }
                const uint64_t hdiff = (__ballot(valid && kme != k0) >> (lane & GSH)) & GMASK;
                if (valid) {
                    Cand& C = L.cand[i];
                    const int32_t m = C.m;
                    if (hdiff == 0) {
                        C.ksel[j] = (NARROW || m <= 16) ? (uint8_t)j : (EQG ? eqg[(m - 17) * BC + j] : s_eqperm[EQG ? 0 : m - 17][EQG ? 0 : j]);
                    } else {
                        int32_t r = 0; bool tie = false;
                        for (int32_t q = 0; q < m; ++q) {
                            const double kq = C.e[q].aux;
                            const bool eq = (kq == kme);
                            const bool before = desc ? (kq > kme) : (kq < kme);
                            r += (before || (eq && q < j)) ? 1 : 0;
                            tie |= (eq && q != j);
                        }
                        r2[k] = r;
                        if (tie) atomicOr(&C.flags, CF_TIE);
                        if (j == 0) atomicOr(&C.flags, CF_NEQ);
                    }
                }
            }
            PHASE_STAMP(17);
            WAVE_SYNC();   // candidate-local: producer and consumer are the same (half-)wave
            PHASE_STAMP(13);
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                if (__ballot(r2[k] >= 0) == 0ull) continue;
                if (r2[k] >= 0) {
                    const int32_t idx = k * NT + tid;
                    Cand& C = L.cand[idx / BCAP];
                    if (NARROW || C.m <= 16 || !(C.flags & CF_TIE)) C.ksel[r2[k]] = (uint8_t)(idx % BCAP);
                }
            }
            if constexpr (BC == 64) {
                // one wave = one candidate: std::sort's permutation with the elements in registers
                WAVE_SYNC();   // candidate-local: producer and consumer are the same (half-)wave   // rank writes of ksel above vs. the sort's own
                int32_t* tmp = L.pslot + (tid >> 6) * 256;   // pslot is not live before the commit
#pragma unroll 1
                for (int k = 0; k < PASSES; ++k) {
                    const int32_t i = k * NWAVE + (tid >> 6);
                    if (i >= ncp) break;
                    Cand& C = L.cand[i];
                    const int32_t fl = C.flags, m = C.m;
                    if ((fl & (CF_BIG | CF_DUP | CF_READY)) || !(m > 16 && (fl & CF_TIE) && (fl & CF_NEQ))) continue;
                    double key = lane < m ? C.e[lane].aux : 0.0;
                    int idx = lane, pos = lane;
                    const WS64 wr = desc ? wave_sort64_call<true>(key, idx, m, lane, tmp) : wave_sort64_call<false>(key, idx, m, lane, tmp);
                    key = wr.key; idx = wr.idx; pos = wr.pos;
                    const bool ok = wr.ok != 0;
                    if (ok) { if (lane < m) C.ksel[pos] = (uint8_t)idx; }
                    else if (lane == 0) { Arrays A3 = A; cand_order_index_call(A3, C); }
                    WAVE_SYNC();
                }
            } else if constexpr (BC == 32) {
                // half a wave = one candidate: the same with two independent sorts per wave
                WAVE_SYNC();   // candidate-local: producer and consumer are the same (half-)wave   // rank writes of ksel above vs. the sort's own
                int32_t* tmp = L.pslot + (tid >> 6) * 256;   // pslot is not live before the commit
#pragma unroll 1
                for (int k = 0; k < PASSES; ++k) {
                    const int32_t i = (k * NT + tid) / BCAP;
                    const int gl = lane & (BC - 1);
                    bool want = false;
                    int32_t m = 0;
                    if (i < ncp) {
                        const int32_t fl = L.cand[i].flags;
                        m = L.cand[i].m;
                        want = !(fl & (CF_BIG | CF_DUP | CF_READY)) && m > 16 && (fl & CF_TIE) && (fl & CF_NEQ);
                    }
                    if (__ballot(want) == 0ull) continue;
                    Cand& C = L.cand[i < ncp ? i : 0];
                    double key = (want && gl < m) ? C.e[gl].aux : 0.0;
                    int idx = gl, pos = gl;
                    const bool ok = desc ? group_sort<true, BC>(key, idx, m, want, lane, tmp, &pos) : group_sort<false, BC>(key, idx, m, want, lane, tmp, &pos);
                    if (want) {
                        if (ok) { if (gl < m) C.ksel[pos] = (uint8_t)idx; }
                        else if (gl == 0) { Arrays A3 = A; cand_order_index_call(A3, C); }
                    }
                    WAVE_SYNC();
                }
            }
            // (16 slots: m <= 16, the stable rank above is std::sort's order)
            WAVE_SYNC();   // candidate-local: producer and consumer are the same (half-)wave
            PHASE_STAMP(14);
            // apply the permutation: every position fetches its source entry, then all store
            double pv[PASSES]; int32_t pn[PASSES], pt[PASSES]; bool pa[PASSES];
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int32_t idx = k * NT + tid;
                const int32_t i = idx / BCAP, j = idx % BCAP;
                pa[k] = (i < ncp) && !(L.cand[i].flags & (CF_BIG | CF_DUP | CF_READY)) && (j < L.cand[i].m);
                pv[k] = 0; pn[k] = 0; pt[k] = 0;
                if (__ballot(pa[k]) == 0ull) continue;
                if (pa[k]) {
                    const Ent& Sx = L.cand[i].e[L.cand[i].ksel[j]]; pv[k] = Sx.val; pn[k] = Sx.nbr; pt[k] = Sx.twin;
                    if (j == 0) { const int32_t m = L.cand[i].m; L.cand[i].ndraw = (A.o_v == OV_COARSEN) ? 1 : (m > 1 ? m - 1 : 0); }   // m >= 1 here
                }
            }
            WAVE_SYNC();   // candidate-local: producer and consumer are the same (half-)wave
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                if (__ballot(pa[k]) == 0ull) continue;
                if (pa[k]) {
                    const int32_t idx = k * NT + tid;
                    Ent& E = L.cand[idx / BCAP].e[idx % BCAP];
                    E.val = pv[k]; E.nbr = pn[k]; E.twin = pt[k]; E.aux = 0;
                }
            }
            }   // BC <= 64
        }
        BSYNC();
        PHASE_STAMP(1);
        // targets shared by several candidates are found with an LDS hash table (keys over pslot, counts over the
        // move arrays: both idle until the commit); cleared here, filled and read in P4 behind later barriers
        int32_t* const hkeys = L.pslot;
        int32_t* const hcnt = L.hcnt;
#pragma unroll
        for (int k = 0; k < PASSES; ++k) { hkeys[k * NT + tid] = -1; hcnt[k * NT + tid] = 0; }
        if (tid < BATCH) L.cmask[tid] = 0ull;
        // ================= P1b: first candidate that depends on an earlier one =================
        if (tid < nc && (L.cand[tid].flags & (CF_BIG | CF_DUP))) atomicMin(&s_pmax, tid);   // (multi-edges show up during the sorts)
        // RNG offsets (P2): a prefix sum does not depend on what follows it, so it is taken over all candidates of the round
        int dtot;
        const int dex = block_excl_scan<NWAVE>((tid < nc && !first_is_big) ? L.cand[tid].ndraw : 0, L.scan, &dtot);
        BSYNC();
        int32_t Pmax = first_is_big ? 0 : (s_pmax < nc ? s_pmax : nc);
        int32_t P = 0;
        PHASE_STAMP(2);
        if (Pmax > 0) {
            // (dtot covers the whole round: at most 4k uniforms more than the prefix needs; the table has that slack)
            if (G.n_draws + dtot > A.rng_len) { if (tid == 0) s_status = ST_RNG_OVERFLOW; BSYNC(); break; }
            // ================= P3: sampling =================
            if (tid < Pmax) {
                L.cand[tid].draw0 = G.n_draws + dex;
                if (!PATCH || L.cand[tid].ndep == 0) cand_cumsum(A, L.cand[tid]);
            }
            BSYNC();
            if (A.o_v != OV_COARSEN) {
                #pragma unroll 1
                for (int k = 0; k < PASSES; ++k) {   // slot-major pairs, rolled (code size): waves whose candidates are short skip later passes
                    const int32_t i = tid / (NT / BATCH), j = k * (NT / BATCH) + tid % (NT / BATCH);
                    if (i >= Pmax || (PATCH && L.cand[i].ndep != 0)) continue;
                    if (j < L.cand[i].m - 1) cand_pick(A, L.cand[i], j);
                }
                // the recurrence (touches e[].val only) runs on the LAST waves, whose share of the picks above is
                // empty unless the round is nearly full: it overlaps with the other waves' picks
                if (tid >= NT - BATCH && tid - (NT - BATCH) < Pmax && (!PATCH || L.cand[tid - (NT - BATCH)].ndep == 0)) cand_recur(A, L.cand[tid - (NT - BATCH)]);
            }
            BSYNC();
            PHASE_STAMP(3);
            if constexpr (PATCH) { if (s_anydep) {
                // ---- dependent candidates: patched from the sampled records of the earlier candidates they are adjacent to, ordered
                //      again and sampled, one wave each; a candidate waits until the ones it depends on are through (a chain of
                //      dependent candidates takes one pass of this loop per link).  What cannot be patched cuts the round. ----
                // (sort scratch: 16-slot candidates order with a stable rank in registers and need none)
                int32_t* const ptmp = NARROW ? nullptr : reinterpret_cast<int32_t*>(L.cont) + (tid >> 6) * 160;   // the record lists are idle until the replay
                static_assert(NARROW || sizeof(CRec) * CCAP * 2 >= (size_t)NWAVE * 160 * 4, "sort scratch of the patching waves fits the record lists");
                // No workgroup barrier per link of a chain: a wave takes its candidates in increasing order and spins on the flags of
                // the (smaller) dependent candidates it needs; the smallest unresolved one can always proceed, so every wave gets through.
                #pragma unroll 1
                for (int32_t i = (tid >> 6); i < Pmax; i += NWAVE) {
                    Cand& C = L.cand[i];
                    const int32_t nd = C.ndep;
                    if (nd == 0) continue;     // (wave-uniform)
                    bool lost = false;
                    for (int32_t q = 0; q < nd && q < DEPMAX; ++q) {
                        Cand& J = L.cand[C.dep[q]];
                        if (J.ndep == 0) continue;
                        volatile int32_t* fp = &J.flags;
                        int32_t f = *fp, spins = 0;
                        while (!(f & (CF_PATCHED | CF_DEP))) {
                            __builtin_amdgcn_s_sleep(1);
                            if (++spins > SPIN_LIMIT) { f = CF_DEP; if (lane == 0) s_status = ST_INTERNAL; break; }   // (a stuck wave must not hang the device -- and must not pass for a result)
                            f = *fp;
                        }
                        if (f & CF_DEP) lost = true;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    if (i >= *(volatile int32_t*)&s_pmax) lost = true;     // behind a cut already
                    bool okp = false;
                    if (!lost) okp = wave_patch<ON>(A.o_v, A.shuffle_seed, A.rng, A.rng_mode, L.cand, i, G.vbase, ptmp);
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    if (lane == 0) {
                        if (okp) { atomicOr(&C.flags, CF_PATCHED); s_npatched = 1; }
                        else { atomicOr(&C.flags, CF_DEP); atomicMin(&s_pmax, i); }
                    }
                }
                BSYNC();
                Pmax = s_pmax < Pmax ? s_pmax : Pmax;
            } }
            if constexpr (PATCH) { if (s_status) break; }   // (workgroup-uniform: read behind the barrier above or the one that ended P3)
            PHASE_STAMP(19);
            PHASE_STAMP(3);
            // ================= P4: PQ replay; targets shared by several candidates go in candidate order =================
            int32_t key0k[PASSES];   // the targets' keys: fetched here, used after the barrier (their latency hides behind the table)
            int32_t tck[PASSES];     // 16-slot shape: my targets' places in the table, then their counts
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int32_t i = PI(k), j = PJ(k);
                key0k[k] = 1;
                if constexpr (NARROW) tck[k] = -1;
                if (i >= Pmax) continue;
                if (j < L.cand[i].m) {
                    if constexpr (SKIP) {
                        // the key-independent half of the replay first: it says whether this pair touches its target at all.  Parked in
                        // the pair's record (not kept in registers across the barrier); an untouched pair is done here -- no key, no
                        // place in the table -- and its record reads "nothing happens" to the commit
                        Cand& C = L.cand[i];
                        int c0, li0;
                        cand_replay_pre(A, C, j, &c0, &li0);
                        TRes& R = ent_tres(C.e[j]);
                        R.key_after = 0; R.flags = 0;
                        if (!cand_touches(OV, C.m, j, C.koff, c0)) { R.c = 0; R.mv = -1; continue; }
                        R.c = (uint8_t)c0; R.mv = (int16_t)li0;
                    }
                    const int32_t x = L.cand[i].e[j].nbr;
                    if (use_pq) key0k[k] = A.vr[x].key;
                    uint32_t hh = ((uint32_t)x * 2654435761u) >> (32 - HBITS);
                    uint32_t step = 0;
                    while (true) {   // open addressing, at most SLOTS distinct keys in SLOTS places; linear probing except in the 16-slot shape
                        const int32_t cur = hkeys[hh];
                        if (cur == x) break;
                        if (cur == -1) { const int32_t old = atomicCAS(&hkeys[hh], -1, x); if (old == -1 || old == x) break; }
                        // (16-slot shape: 192 candidates fill the table to 0.47 and nobody looks a key up again -- the place is kept in tck --
                        // so the probe sequence is the triangular one, which visits every place of a power-of-two table without
                        // the runs linear probing builds)
                        if constexpr (NARROW) { ++step; hh = (hh + step) & (SLOTS - 1); }
                        else hh = (hh + 1) & (SLOTS - 1);
                    }
                    atomicAdd(&hcnt[hh], 1);
                    if constexpr (NARROW) tck[k] = (int32_t)hh;
                }
            }
            BSYNC();
            PHASE_STAMP(33);
            // 16-slot shape: twice the candidates share half the record list, and small graphs (hubs) fill it in most rounds.  A
            // record's place is therefore not the order of arrival (the first record that finds the list full may belong to ANY
            // candidate, and the round ends in front of it) but the candidate order: the round keeps every candidate whose records
            // fit.  Counts per thread -> per candidate (four adjacent lanes) -> prefix over the wave's 16 candidates -> over the waves.
            int32_t crec = 0;   // place of my next contended record
            if constexpr (NARROW) {
                int mine_c = 0;
#pragma unroll
                for (int k = 0; k < PASSES; ++k) {
                    tck[k] = tck[k] >= 0 ? hcnt[tck[k]] : 0;
                    mine_c += tck[k] > 1 ? 1 : 0;
                }
                const int l4 = lane & 3, l0 = lane & ~3;
                const int c0 = __shfl(mine_c, l0), c1 = __shfl(mine_c, l0 + 1), c2 = __shfl(mine_c, l0 + 2), c3 = __shfl(mine_c, l0 + 3);
                const int csum = c0 + c1 + c2 + c3;
                const int before_me = (l4 > 0 ? c0 : 0) + (l4 > 1 ? c1 : 0) + (l4 > 2 ? c2 : 0);
                int incl = l4 == 0 ? csum : 0;
                for (int off = 1; off < 64; off <<= 1) { int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
                if (lane == 63) L.scan[tid >> 6] = incl;
                BSYNC();
                int wbase = 0;
                for (int w = 0; w < (tid >> 6); ++w) wbase += L.scan[w];
                crec = wbase + incl - csum + before_me;
                if (tid == NT - 1) s_ncont = wbase + incl;
            }
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int32_t i = PI(k), j = PJ(k);
                uint64_t pm = 0ull;
                if constexpr (GROUPED) {
                    if (__ballot(i < Pmax) == 0ull) continue;   // (wave-uniform)
                    const bool cok = i < Pmax;
                    pm = group_pick_mask<BC <= 64 ? BC : 64>(L.cand[cok ? i : 0].ksel, cok ? L.cand[i].m : 0, cok, lane);
                }
                if (i >= Pmax) continue;
                if constexpr (NARROW) { if (tck[k] == 0) continue; }   // no such position, or an untouched pair: its count was never taken
                Cand& C = L.cand[i];
                if (j >= C.m) continue;
                TRes& R = ent_tres(C.e[j]);
                // an untouched pair is not in the table (the look-up below would never end for it): before anything else
                if constexpr (SKIP && !NARROW) { if (!cand_touches(OV, C.m, j, C.koff, (int)R.c)) continue; }
                const int32_t x = C.e[j].nbr;
                int32_t tc;
                if constexpr (NARROW) tc = tck[k];
                else {
                    uint32_t hh = ((uint32_t)x * 2654435761u) >> (32 - HBITS);
                    while (hkeys[hh] != x) hh = (hh + 1) & (SLOTS - 1);
                    tc = hcnt[hh];
                }
                const int32_t key0 = key0k[k];
                if (tc > 1) {
                    // the key-independent half of the replay is done (P4.1, or here, in parallel); the walk below chains the keys
                    if constexpr (SKIP) R.flags = TF_CONTENDED;
                    else {
                        int c0, li0;
                        if constexpr (GROUPED) { c0 = __popcll(pm); li0 = pm ? 63 - __builtin_clzll(pm) : -1; }
                        else cand_replay_pre(A, C, j, &c0, &li0);
                        R.flags = TF_CONTENDED; R.mv = (int16_t)li0; R.c = (uint8_t)c0; R.key_after = 0;
                    }
                    int32_t q;
                    if constexpr (NARROW) q = crec++; else q = atomicAdd(&s_ncont, 1);
                    if (q < CCAP) { L.cont[q].x = x; L.cont[q].i = i; L.cont[q].j = j; }
                    else atomicMin(&s_p, i);     // record list full: stop the round before this candidate
                    continue;
                }
                const bool allow_last = (done + i + 1) + 1 < (int64_t)n;
                int mv, c; bool cx = false;
                int32_t k2;
                if constexpr (GROUPED) {
                    c = __popcll(pm);
                    k2 = cand_replay_post(A, C, j, key0, use_pq ? n : 0x7FFFFFFF, allow_last, c, pm ? 63 - __builtin_clzll(pm) : -1, &mv, &cx);
                } else if constexpr (SKIP) {
                    c = (int)R.c;
                    k2 = cand_replay_post(A, C, j, key0, use_pq ? n : 0x7FFFFFFF, allow_last, c, (int)R.mv, &mv, &cx);
                } else k2 = cand_replay(A, C, j, key0, use_pq ? n : 0x7FFFFFFF, allow_last, &mv, &c, &cx);
                if (!use_pq) { mv = -1; cx = false; }
                R.key_after = k2; R.mv = (int16_t)mv; R.c = (uint8_t)c; R.flags = 0;
                if (cx) atomicMin(&s_p, i);   // keys beyond n: this candidate goes to the single-vertex path
                if (mv >= 0) {
                    atomicAdd(&C.nmv, 1);
                    if (pq_list_of(k2, n) <= G.minlist) atomicMin(&s_p, i + 1);   // pre-empts the predicted order: last of the round
                }
            }
            BSYNC();
            PHASE_STAMP(34);
            // contended records: order by (x, i) with a rank sort (keys are distinct), then replay each group in order
            const int32_t ncont = s_ncont < CCAP ? s_ncont : CCAP;
            CRec* csorted = L.csorted;
            for (int32_t q = tid; q < ncont; q += NT) {
                CRec me = L.cont[q];
                uint64_t kme = ((uint64_t)(uint32_t)me.x << 32) | (uint32_t)me.i;
                int rank = 0;
                for (int32_t r = 0; r < ncont; ++r) {
                    uint64_t kr = ((uint64_t)(uint32_t)L.cont[r].x << 32) | (uint32_t)L.cont[r].i;
                    rank += (kr < kme) ? 1 : 0;
                }
                csorted[rank] = me;
            }
            BSYNC();
            PHASE_STAMP(35);
            for (int32_t q = tid; q < ncont; q += NT) {
                if (q > 0 && csorted[q - 1].x == csorted[q].x) continue;   // group head only
                int32_t x = csorted[q].x;
                int32_t key = use_pq ? A.vr[x].key : 1;
                for (int32_t r = q; r < ncont && csorted[r].x == x; ++r) {
                    Cand& C = L.cand[csorted[r].i];
                    const bool allow_last = (done + csorted[r].i + 1) + 1 < (int64_t)n;
                    TRes& R = ent_tres(C.e[csorted[r].j]);
                    int mv; bool cx = false;
                    int32_t k2 = cand_replay_post(A, C, csorted[r].j, key, use_pq ? n : 0x7FFFFFFF, allow_last, (int)R.c, (int)R.mv, &mv, &cx);
                    if (!use_pq) { mv = -1; cx = false; }
                    R.key_after = k2; R.mv = (int16_t)mv;
                    if (cx) atomicMin(&s_p, csorted[r].i);
                    if (mv >= 0) {
                        atomicAdd(&C.nmv, 1);
                        if (pq_list_of(k2, n) <= G.minlist) atomicMin(&s_p, csorted[r].i + 1);
                    }
                    key = k2;
                }
            }
            BSYNC();
            // ================= P: the first pre-empting / complex candidate was noted during the replay; bound the
            PHASE_STAMP(36);
            // number of moves (candidates sit in the first BATCH / 64 waves: a wave scan and their totals through LDS) =================
            {
                const int mycnt = tid < Pmax ? L.cand[tid].nmv : 0;
                int incl = mycnt;
                for (int off = 1; off < 64; off <<= 1) { int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
                constexpr int CW = (BATCH + 63) / 64;   // waves that hold candidates
                static_assert(CW <= 4 && CW <= NWAVE, "candidates live in the first waves");
                if (lane == 63 && (tid >> 6) < CW - 1) L.scan[tid >> 6] = incl;
                BSYNC();
                int before = 0;
#pragma unroll
                for (int w = 0; w < CW - 1; ++w) before += (w < (tid >> 6)) ? L.scan[w] : 0;
                if (tid < Pmax && incl + before > MCAP) atomicMin(&s_p, tid);
            }
            BSYNC();
            P = s_p < Pmax ? s_p : Pmax;
            PHASE_STAMP(4);
        }
        if (P == 0) {
            // ================= single-vertex path for candidate 0 =================
            ++singles;
            const int32_t v0 = L.cand[0].v, src0 = L.cand[0].src;
            BSYNC();
            if (tid < nc) batch_pos[L.cand[tid].v] = -1;
            if (tid == 0 && use_pq) {
                if (src0 >= 0) A.bs_cnt[b] = src0; else { A.bs_cnt[b] = 0; A.ocur[b] = (~src0) + 1; }
                A.vr[v0].pqpos = -2;
            }
            BSYNC();
            if (tid < 64) {
                // the out-of-line paths take the descriptors by reference: hand them private copies so that
                // the kernel's own copy never has its address taken (it would otherwise live in scratch
                // memory and every A.member access in the hot phases would be a scratch load)
                Arrays A2 = A;
                ElimScratch S2 = S;
                int32_t cp0 = A2.colptr[v0], cp1 = A2.colptr[v0 + 1];
                int32_t acnt = A2.vr[v0].app_cnt, abase = A2.vr[v0].app_chunk;
                if ((cp1 - cp0) + acnt > EC1) {
                    bool handled = false;
                    if (OV == OV_RANDOM) {
                        ColBuf Bf = S2.colbuf(G.scr_base);
                        handled = wave_eliminate_big(A2, G, sh.g, Bf, G.scr_cap, v0, cp0, cp1, acnt, abase, s_help);
                    }
                    if (!handled && lane == 0) {
                        __hip_atomic_store(&s_help[0], 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);   // (before, not after: see above)
                        serial_eliminate_call(A2, G, S2, v0, done + 1);
                    }
                } else {
                    wave_eliminate(A2, G, sh.e, v0, done + 1, cp0, cp1, acnt, abase, (S.prof && g == 0) ? &s_prof[24] : nullptr, s_help);
                }
            } else if (tid < 128) {
                single_helper(sh.e, sh.g.c.newv, s_help);
            }
            if (tid == 0) { s_nc = 0; s_pmax = BATCH + 1; s_p = BATCH + 1; s_ncont = 0; s_nmoves = 0; s_anydep = 0; s_npatched = 0; s_dirb = -1; }
            BSYNC();
            if (G.status != 0 || s_help[2] != 0) { if (tid == 0) s_status = G.status ? G.status : ST_INTERNAL; BSYNC(); break; }
            done += 1;
            PHASE_STAMP(5);
            continue;
        }

        // ================= P5: commit candidates [0,P) =================
        if (tid == 0 && use_pq) {
            int32_t src = L.cand[P - 1].src;
            if (src >= 0) A.bs_cnt[b] = src; else { A.bs_cnt[b] = 0; A.ocur[b] = (~src) + 1; }
        }
        int32_t status = 0;
        if (tid < P) {
            Cand& C = L.cand[tid];
            if (use_pq) A.vr[C.v].pqpos = -2;
            // the edge to the last neighbour (or to the coarsening target) dies (:429-430 | :880-881)
            if (C.m >= 1) {
                const int32_t tw = C.e[A.o_v == OV_COARSEN ? C.koff : C.m - 1].twin;
                if (!PATCH || tw >= 0) A.e[tw].val = 0;   // (a patched entry's twin is appended in this very round: second pass of the rewire stores)
            }
            if (MERGE) for (int32_t q = 0; q < C.nkill; ++q) A.e[C.e[C.m + q].twin].val = 0;   // merged multi-edges (:289)
        }
        // append cursors of the targets shared by several candidates: loaded now (one group head per thread), used
        // after the pool bump below
        const int32_t ncont_c = s_ncont < CCAP ? s_ncont : CCAP;
        bool chead = false;
        int32_t ca0 = 0, cchunk0 = 0;
        if (tid < ncont_c) {
            const CRec me = L.csorted[tid];
            chead = (tid == 0 || L.csorted[tid - 1].x != me.x) && me.i < P;
            if (chead) { ca0 = A.vr[me.x].app_cnt; cchunk0 = A.vr[me.x].app_chunk; }
            // which positions of candidate me.i push into this target: found here by every record's own thread, so that
            // the group walk below only steps through the set bits (the unsorted record list is free: used as scratch)
            uint64_t pm = 0ull, pm_hi = 0ull;
            if (me.i < P) {
                const Cand& C = L.cand[me.i];
                if (BC <= 64 && A.o_v == OV_COARSEN) { if (me.j == C.koff) pm = ((C.m >= 64 ? ~0ull : ((1ull << C.m) - 1ull)) & ~(1ull << C.koff)); }
                else for (int32_t w = 0; 8 * w < C.m - 1; ++w) {
                    for (uint64_t y = ksel_matches(C.ksel, w, me.j, C.m - 1); y; y &= y - 1) {
                        const int32_t p = 8 * w + (ctz_u64(y) >> 3);
                        if (BC <= 64 || p < 64) pm |= 1ull << (p & 63); else pm_hi |= 1ull << (p & 63);
                    }
                }
            }
            L.cont[tid].x = (int32_t)(uint32_t)pm; L.cont[tid].j = (int32_t)(uint32_t)(pm >> 32);
            if (BC == 128) L.mkey[tid] = pm_hi;   // (128-slot candidates: o_v = random only, no PQ moves -- the move list is free)
        }
        // targets touched by one candidate only: one thread per (candidate, target); two passes so that
        // all loads are in flight together and the pool is bumped once per round
        {
            TRes Rk[PASSES]; int32_t xk[PASSES], a0k[PASSES], chk[PASSES], needk[PASSES]; bool actk[PASSES];
            int32_t need_thread = 0;
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int32_t i = PI(k), j = PJ(k);
                actk[k] = false; xk[k] = 0; a0k[k] = 0; chk[k] = -1; needk[k] = 0;
                Rk[k].key_after = 0; Rk[k].mv = -1; Rk[k].c = 0; Rk[k].flags = 0;
                if (i < P && j < L.cand[i].m) {
                    Rk[k] = ent_tres(L.cand[i].e[j]);
                    xk[k] = L.cand[i].e[j].nbr;
                    actk[k] = !(Rk[k].flags & TF_CONTENDED);
                }
                if (actk[k] && Rk[k].c > 0) { a0k[k] = A.vr[xk[k]].app_cnt; chk[k] = A.vr[xk[k]].app_chunk; }
            }
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                if (__ballot(actk[k] && Rk[k].c > 0) != 0ull && actk[k] && Rk[k].c > 0) {
                    for (int32_t t = 0; t < (int32_t)Rk[k].c; ++t) {
                        int32_t a = a0k[k] + t;
                        int c = chunk_of(a);
                        if (a == chunk_start(c)) needk[k] += 1 + chunk_cap(c);
                    }
                }
                need_thread += needk[k];
            }
            int ntot;
            int nex = block_excl_scan<NWAVE>(need_thread, L.scan, &ntot);
            if (tid == 0) {
                // slots come from a reservation this workgroup holds (refilled with one global atomic when it
                // runs out): the round does not wait for a device-wide atomic
                int32_t base = 0;
                if (ntot > 0) {
                    if (s_pool_cur + ntot > s_pool_end) {
                        const int32_t grab = ntot > POOL_GRAB ? ntot : POOL_GRAB;
                        const int32_t b0 = atomicAdd(A.pool_top, grab);
                        if (b0 < 0 || b0 > A.slot_cap - grab) { s_pool_cur = 0; s_pool_end = 0; base = -1; }
                        else { s_pool_cur = b0; s_pool_end = b0 + grab; }
                    }
                    if (base == 0) { base = s_pool_cur; s_pool_cur += ntot; }
                }
                L.scan[NWAVE + 1] = base;
            }
            BSYNC();
            const int32_t pbase = L.scan[NWAVE + 1];
            if (pbase < 0) status = ST_POOL_OVERFLOW;
            PHASE_STAMP(10);
            int32_t cursor = pbase + nex;
#pragma unroll
            for (int k = 0; k < PASSES; ++k) {
                const int32_t i = PI(k), j = PJ(k);
                if (__ballot(actk[k]) == 0ull) continue;
                uint64_t pm = 0ull;
                if constexpr (GROUPED) {
                    const bool cok = i < P;
                    pm = group_pick_mask<BC <= 64 ? BC : 64>(L.cand[cok ? i : 0].ksel, cok ? L.cand[i].m : 0, cok, lane);
                }
                if (actk[k] && Rk[k].c > 0 && status == 0) {
                    const Cand& C = L.cand[i];
                    int32_t a = a0k[k], chunk = chk[k];
                    if constexpr (GROUPED) {
                        for (uint64_t mm = pm; mm; mm &= mm - 1) {   // the positions that push into this target, ascending
                            const int p = __builtin_ctzll(mm);
                            int c = chunk_of(a);
                            int32_t cs = chunk_start(c);
                            if (a == cs) { A.e[cursor].nbr = chunk; chunk = cursor; cursor += 1 + chunk_cap(c); }
                            L.pslot[i * BCAP + p] = chunk + 1 + (a - cs);
                            ++a;
                        }
                    } else {
                    if (A.o_v == OV_COARSEN) {
                        for (int32_t p = 0; p < C.m; ++p) {
                            if (p == C.koff) continue;
                            int c = chunk_of(a);
                            int32_t cs = chunk_start(c);
                            if (a == cs) { A.e[cursor].nbr = chunk; chunk = cursor; cursor += 1 + chunk_cap(c); }
                            L.pslot[i * BCAP + p] = chunk + 1 + (a - cs);
                            ++a;
                        }
                    } else {
                        for (int32_t w = 0; 8 * w < C.m - 1; ++w) {   // the picks that name this target, eight per load, ascending
                            for (uint64_t y = ksel_matches(C.ksel, w, j, C.m - 1); y; y &= y - 1) {
                                const int32_t p = 8 * w + (ctz_u64(y) >> 3);
                                int c = chunk_of(a);
                                int32_t cs = chunk_start(c);
                                if (a == cs) { A.e[cursor].nbr = chunk; chunk = cursor; cursor += 1 + chunk_cap(c); }
                                L.pslot[i * BCAP + p] = chunk + 1 + (a - cs);
                                ++a;
                            }
                        }
                    }
                    }
                    A.vr[xk[k]].app_cnt = a; A.vr[xk[k]].app_chunk = chunk;
                }
                const bool mvd = use_pq && actk[k] && Rk[k].mv >= 0;
                const uint64_t mvmask = __ballot(mvd);
                int32_t qbase = 0;
                if (mvmask) {   // one LDS atomic per wave instead of one per move
                    if (lane == __builtin_ctzll(mvmask)) qbase = atomicAdd(&s_nmoves, __popcll(mvmask));
                    qbase = __shfl(qbase, __builtin_ctzll(mvmask));
                }
                if (mvd) {
                    A.vr[xk[k]].key = Rk[k].key_after;
                    atomicOr(&L.cmask[i], 1ull << (Rk[k].mv - L.cand[i].m));
                    int32_t q = qbase + __popcll(mvmask & lanemask_lt(lane));
                    if (q < MCAP) {
                        L.mkey[q] = ((uint64_t)(uint32_t)pq_list_of(Rk[k].key_after, n) << 32) | (uint32_t)((i << SEQSH) | Rk[k].mv);
                        L.mval[q] = xk[k];
                    }
                }
            }
        }
        PHASE_STAMP(37);
        // targets shared by several candidates: one thread walks the target's records in candidate order
        {
            const int32_t ncont = ncont_c;   // <= CCAP < NT: one record per thread
            const CRec* csorted = L.csorted;
            if (chead) {
                const int32_t q = tid;
                const int32_t x = csorted[q].x;
                int32_t a = ca0, chunk = cchunk0;
                const int32_t a_before = a;
                int32_t key_final = 0, mvseq = -1;
                for (int32_t r = q; r < ncont && csorted[r].x == x && csorted[r].i < P; ++r) {
                    Cand& C = L.cand[csorted[r].i];
                    int32_t* pslot_row = &L.pslot[csorted[r].i * BCAP];
                    uint64_t pm = ((uint64_t)(uint32_t)L.cont[r].j << 32) | (uint32_t)L.cont[r].x;
                    while (pm && status == 0) { const int p = __builtin_ctzll(pm); pm &= pm - 1; pslot_row[p] = alloc_in_column(A, a, chunk, &status); }
                    if constexpr (BC == 128) {
                        uint64_t ph = L.mkey[r];
                        while (ph && status == 0) { const int p = __builtin_ctzll(ph); ph &= ph - 1; pslot_row[64 + p] = alloc_in_column(A, a, chunk, &status); }
                    }
                    TRes R = ent_tres(C.e[csorted[r].j]);
                    key_final = R.key_after;
                    if (R.mv >= 0) mvseq = (csorted[r].i << SEQSH) | R.mv;
                }
                if (a != a_before) { A.vr[x].app_cnt = a; A.vr[x].app_chunk = chunk; }
                if (use_pq) {
                    A.vr[x].key = key_final;
                    if (mvseq >= 0) {
                        atomicOr(&L.cmask[mvseq >> SEQSH], 1ull << ((mvseq & ((1 << SEQSH) - 1)) - L.cand[mvseq >> SEQSH].m));
                        int32_t qq = atomicAdd(&s_nmoves, 1);
                        if (qq < MCAP) {
                            L.mkey[qq] = ((uint64_t)(uint32_t)pq_list_of(key_final, n) << 32) | (uint32_t)mvseq;
                            L.mval[qq] = x;
                        }
                    }
                }
            }
        }
        if (__syncthreads_or(status != 0)) { if (tid == 0) s_status = ST_POOL_OVERFLOW; BSYNC(); break; }
        if (S.jitter > 0 && ((threadIdx.x >> 6) & 1)) for (int _q = 0; _q < S.jitter; ++_q) __builtin_amdgcn_s_sleep(8);
        PHASE_STAMP(6);
        // one thread per appended entry: twin rewritten in place + the new entry (:404-414)
#pragma unroll
        for (int k = 0; k < PASSES; ++k) {
            const int32_t i = tid / (NT / BATCH), pp = k * (NT / BATCH) + tid % (NT / BATCH);
            if (i < P) {
                const Cand& C = L.cand[i];
                const bool co = A.o_v == OV_COARSEN;
                if (co ? (pp < C.m && pp != C.koff) : (pp < C.m - 1)) {
                    const int32_t kk = co ? C.koff : (int32_t)C.ksel[pp];
                    if (!PATCH || C.e[pp].twin >= 0) rewire_store(A, C.e[pp].twin, L.pslot[i * BCAP + pp], C.e[pp].nbr, C.e[kk].nbr, C.e[pp].val);
                }
            }
        }
        if (PATCH && s_npatched) {
            // entries of patched candidates whose twin is an entry an EARLIER candidate of this round appends (~twin = its place in the
            // slot table): that candidate's stores (first pass, above) come first, the rewrite in place (:404-406) or the kill (:429-430) second
            BSYNC();
#pragma unroll 1
            for (int k = 0; k < PASSES; ++k) {
                const int32_t i = tid / (NT / BATCH), pp = k * (NT / BATCH) + tid % (NT / BATCH);
                if (i < P) {
                    const Cand& C = L.cand[i];
                    if (pp < C.m && C.e[pp].twin < 0) {
                        const int32_t s_r = L.pslot[~C.e[pp].twin];
                        if (pp < C.m - 1) rewire_store(A, s_r, L.pslot[i * BCAP + pp], C.e[pp].nbr, C.e[(int32_t)C.ksel[pp]].nbr, C.e[pp].val);
                        else A.e[s_r].val = 0;
                    }
                }
            }
        }
        PHASE_STAMP(11);
        const int32_t nmoves = s_nmoves;
        if (nmoves > MCAP) { if (tid == 0) s_status = ST_INTERNAL; BSYNC(); break; }
        if (use_pq && nmoves > 0) {
            static_assert(BC <= 32 || OV == OV_RANDOM, "op numbers mv - m fit a 64-bit mask for candidates of up to 32 slots");
            // ---- order of the moves = (bucket, candidate, op).  No sort: a move's place in (candidate, op) order is
            //      the candidates' move counts summed before it plus the rank of its op bit in its candidate's mask;
            //      the moves are laid out in that order, then each finds its rank inside its bucket by counting
            //      (64 buckets above the lowest through a per-wave table, the few beyond -- hubs -- by comparing
            //      among themselves).  Falls back to the bitonic sort when more than 128 moves go beyond. ----
            const bool mine = tid < nmoves;
            int32_t list_my = 0, x_my = -1, rank_my = 0, pos_my = 0;
            bool tail_my = false;
            uint32_t bmin = 0xFFFFFFFFu;
            bool fallback = false;
            {
                const uint64_t kq0 = mine ? L.mkey[tid] : 0ull;
                const int32_t x0 = mine ? L.mval[tid] : -1;
                const int32_t seq = (int32_t)(kq0 & 0x7FFFull);
                const int32_t ci = seq >> SEQSH, cmv = seq & ((1 << SEQSH) - 1);
                if (mine) bmin = (uint32_t)(kq0 >> 32);
                for (int off = 32; off > 0; off >>= 1) bmin = min(bmin, (uint32_t)__shfl_xor((int)bmin, off));
                if (lane == 0) L.scan[tid >> 6] = (int32_t)bmin;
                const int cnt_i = tid < P ? __popcll(L.cmask[tid]) : 0;
                int incl = cnt_i;
                for (int off = 1; off < 64; off <<= 1) { int t = __shfl_up(incl, off); if (lane >= off) incl += t; }
                constexpr int CW = (BATCH + 63) / 64;   // waves that hold candidates (their totals: L.scan[NWAVE ..])
                if (lane == 63 && (tid >> 6) < CW - 1) L.scan[NWAVE + (tid >> 6)] = incl;
                BSYNC();
                for (int w = 0; w < NWAVE; ++w) bmin = min(bmin, (uint32_t)L.scan[w]);
                int cbefore = 0;
#pragma unroll
                for (int w = 0; w < CW - 1; ++w) cbefore += (w < (tid >> 6)) ? L.scan[NWAVE + w] : 0;
                if (tid < P) L.hidx[tid] = incl - cnt_i + cbefore;
                // [NWAVE][RB] move counts per (wave, bucket above the lowest); pslot is idle now (SLOTS = NWAVE * 256 ints)
                constexpr int RB = 256, HCAP = 128;
                static_assert(NWAVE * RB <= SLOTS && 2 * RB + 2 * HCAP <= 3 * CCAP * 2, "tables fit pslot / the record lists");
                int32_t* const wtab = L.pslot;
#pragma unroll
                for (int k = 0; k < PASSES; ++k) wtab[k * NT + tid] = 0;
                if (tid == 0) s_nhigh = 0;
                BSYNC();
                uint32_t* const lst32 = reinterpret_cast<uint32_t*>(L.mkey);
                if (mine) {
                    const int32_t idx = L.hidx[ci] + __popcll(L.cmask[ci] & ((1ull << (cmv - L.cand[ci].m)) - 1ull));
                    lst32[idx] = (uint32_t)(kq0 >> 32);
                    L.mval[idx] = x0;
                }
                BSYNC();
                if (mine) { list_my = (int32_t)lst32[tid]; x_my = L.mval[tid]; }
                const uint32_t brel = (uint32_t)list_my - bmin;
                const bool low = mine && brel < (uint32_t)RB, high = mine && brel >= (uint32_t)RB;
                int32_t* const btot = reinterpret_cast<int32_t*>(L.cont);     // [RB] moves per low bucket (the record lists are idle now)
                int32_t* const bstart = btot + RB;                            // [RB] first sorted position of a low bucket
                int32_t* const hl_list = bstart + RB;                         // [HCAP] buckets of the moves beyond
                int32_t* const hl_idx = hl_list + HCAP;                       // [HCAP] their places in (candidate, op) order
                int rank_w = 0;
                {
                    // lanes of my wave with my bucket: one ballot per bit of the bucket number (8 bits) instead of a loop
                    // over the distinct buckets of the wave
                    static_assert(RB == 256, "8 bits of bucket number");
                    uint64_t eq = __ballot(low);
#pragma unroll
                    for (int bit = 0; bit < 8; ++bit) {
                        const bool mybit = (brel >> bit) & 1u;
                        const uint64_t bb = __ballot(low && mybit);
                        eq &= mybit ? bb : ~bb;
                    }
                    if (low) {
                        const uint64_t before = eq & lanemask_lt(lane);
                        rank_w = __popcll(before);
                        if (before == 0ull) wtab[(tid >> 6) * RB + brel] = __popcll(eq);
                    }
                }
                if (high) { const int32_t q = atomicAdd(&s_nhigh, 1); if (q < HCAP) { hl_list[q] = list_my; hl_idx[q] = tid; } }
                BSYNC();
                const int32_t nhigh = s_nhigh;
                fallback = nhigh > HCAP;
                if (!fallback) {
                    if (tid < RB) {   // per bucket: exclusive prefix over the waves, total
                        int acc = 0;
                        for (int w = 0; w < NWAVE; ++w) { const int t = wtab[w * RB + tid]; wtab[w * RB + tid] = acc; acc += t; }
                        btot[tid] = acc;
                    }
                    BSYNC();
                    if (tid < 64) {   // bucket starts: each lane of wave 0 takes RB/64 consecutive buckets
                        int tsum = 0;
#pragma unroll
                        for (int u = 0; u < RB / 64; ++u) tsum += btot[tid * (RB / 64) + u];
                        int inc2 = tsum;
                        for (int off = 1; off < 64; off <<= 1) { int t = __shfl_up(inc2, off); if (lane >= off) inc2 += t; }
                        int run = inc2 - tsum;
#pragma unroll
                        for (int u = 0; u < RB / 64; ++u) { bstart[tid * (RB / 64) + u] = run; run += btot[tid * (RB / 64) + u]; }
                        if (tid == 63) s_nlow = inc2;
                    }
                    BSYNC();
                    if (low) {
                        rank_my = wtab[(tid >> 6) * RB + brel] + rank_w;
                        pos_my = bstart[brel] + rank_my;
                        tail_my = rank_my == btot[brel] - 1;
                    } else if (high) {
                        int32_t before = 0, same_b = 0, cntb = 0;
                        for (int32_t q = 0; q < nhigh; ++q) {
                            const int32_t l2 = hl_list[q], t2 = hl_idx[q];
                            before += (l2 < list_my || (l2 == list_my && t2 < tid)) ? 1 : 0;
                            if (l2 == list_my) { ++cntb; same_b += (t2 < tid) ? 1 : 0; }
                        }
                        rank_my = same_b;
                        pos_my = s_nlow + before;
                        tail_my = rank_my == cntb - 1;
                    }
                } else {
                    // the moves sit in (candidate, op) order: their place stands in for the (candidate, op) key
                    BSYNC();
                    L.mkey[tid] = mine ? (((uint64_t)(uint32_t)list_my << 32) | (uint32_t)tid) : ~0ull;
                    L.mval[tid] = x_my;
                    BSYNC();
                }
            }
            if (fallback) {
                // ---- sort the moves by (bucket, op order): bitonic, one element per thread; strides < 64 stay
                //      inside the wave (shuffles), only the larger strides go through LDS.  Keys are packed
                //      into 32 bits ((bucket - lowest bucket) << 15 | candidate << 8 | op) when they fit ----
                {
                    uint64_t kq = tid < nmoves ? L.mkey[tid] : ~0ull;
                    int32_t vq = tid < nmoves ? L.mval[tid] : -1;
                    uint32_t bmin = tid < nmoves ? (uint32_t)(kq >> 32) : 0xFFFFFFFFu, bmax = tid < nmoves ? (uint32_t)(kq >> 32) : 0u;
                    for (int off = 32; off > 0; off >>= 1) { bmin = min(bmin, (uint32_t)__shfl_xor((int)bmin, off)); bmax = max(bmax, (uint32_t)__shfl_xor((int)bmax, off)); }
                    if (lane == 0) { L.scan[tid >> 6] = (int32_t)bmin; L.hidx[tid >> 6] = (int32_t)bmax; }
                    BSYNC();
                    for (int w = 0; w < NWAVE; ++w) { bmin = min(bmin, (uint32_t)L.scan[w]); bmax = max(bmax, (uint32_t)L.hidx[w]); }
                    int32_t npow = 64;
                    while (npow < nmoves) npow <<= 1;
                    BSYNC();
                    if (bmax - bmin < (1u << 16)) {
                        uint32_t k32 = tid < nmoves ? ((((uint32_t)(kq >> 32) - bmin) << 15) | ((uint32_t)kq & 0x7FFFu)) : 0xFFFFFFFFu;
                        uint32_t* lk = reinterpret_cast<uint32_t*>(L.mkey);
                        for (int32_t k = 2; k <= npow; k <<= 1) {
                            for (int32_t jj = k >> 1; jj > 0; jj >>= 1) {
                                const bool take_min = (((tid & jj) == 0) == ((tid & k) == 0));
                                uint32_t ko; int32_t vo;
                                if (jj >= 64) {
                                    lk[tid] = k32; L.mval[tid] = vq;
                                    BSYNC();
                                    ko = lk[tid ^ jj]; vo = L.mval[tid ^ jj];
                                    BSYNC();
                                } else {
                                    ko = (uint32_t)__shfl_xor((int)k32, jj);
                                    vo = __shfl_xor(vq, jj);
                                }
                                const bool swap = take_min ? (ko < k32) : (ko > k32);
                                if (swap) { k32 = ko; vq = vo; }
                            }
                        }
                        BSYNC();
                        kq = (k32 == 0xFFFFFFFFu) ? ~0ull : ((((uint64_t)((k32 >> 15) + bmin)) << 32) | (uint64_t)(k32 & 0x7FFFu));
                    } else {
                        for (int32_t k = 2; k <= npow; k <<= 1) {
                            for (int32_t jj = k >> 1; jj > 0; jj >>= 1) {
                                const bool take_min = (((tid & jj) == 0) == ((tid & k) == 0));
                                uint64_t ko; int32_t vo;
                                if (jj >= 64) {
                                    L.mkey[tid] = kq; L.mval[tid] = vq;
                                    BSYNC();
                                    ko = L.mkey[tid ^ jj]; vo = L.mval[tid ^ jj];
                                    BSYNC();
                                } else {
                                    uint32_t lo32 = (uint32_t)kq, hi32 = (uint32_t)(kq >> 32);
                                    uint32_t olo = (uint32_t)__shfl_xor((int)lo32, jj), ohi = (uint32_t)__shfl_xor((int)hi32, jj);
                                    ko = ((uint64_t)ohi << 32) | olo;
                                    vo = __shfl_xor(vq, jj);
                                }
                                const bool swap = take_min ? (ko < kq) : (ko > kq);
                                if (swap) { kq = ko; vq = vo; }
                            }
                        }
                    }
                    L.mkey[tid] = kq; L.mval[tid] = vq;
                    BSYNC();
                }
                // ---- bucket-group head index of every move (inclusive max scan) ----
                {
                    int32_t carry = 0;
                    for (int32_t c0 = 0; c0 < nmoves; c0 += NT) {
                        int32_t r = c0 + tid;
                        int32_t hv = -1;
                        if (r < nmoves) {
                            uint32_t bk = (uint32_t)(L.mkey[r] >> 32);
                            bool head = (r == 0) || ((uint32_t)(L.mkey[r - 1] >> 32) != bk);
                            hv = head ? r : -1;
                        }
                        int32_t incl = hv;
                        for (int off = 1; off < 64; off <<= 1) { int32_t tt = __shfl_up(incl, off); if (lane >= off) incl = max(incl, tt); }
                        if (lane == 63) L.scan[tid >> 6] = incl;
                        BSYNC();
                        int32_t pre = carry;
                        for (int w = 0; w < (tid >> 6); ++w) pre = max(pre, L.scan[w]);
                        incl = max(incl, pre);
                        if (r < nmoves) L.hidx[r] = incl;
                        int32_t nc2 = carry;
                        for (int w = 0; w < NWAVE; ++w) nc2 = max(nc2, L.scan[w]);
                        carry = nc2;
                        BSYNC();
                    }
                }
                if (mine) {
                    list_my = (int32_t)(L.mkey[tid] >> 32);
                    x_my = L.mval[tid];
                    rank_my = tid - L.hidx[tid];
                    pos_my = tid;
                    tail_my = (tid == nmoves - 1) || ((uint32_t)(L.mkey[tid + 1] >> 32) != (uint32_t)(L.mkey[tid] >> 32));
                    if (tid == 0) bmin = (uint32_t)list_my;
                }
                bmin = (uint32_t)(L.mkey[0] >> 32);
            }
            PHASE_STAMP(7);
            // ---- allocate new stack chunks, then write the entries (one move per thread; the stack height and chunk
            //      count are read once and kept in registers) ----
            int32_t bk = 0, a_my = 0, c_my = 0, al_my = 0;
            if (mine) {
                bk = G.bucket_base + list_my;
                a_my = A.bs_cnt[bk] + rank_my;
                al_my = A.bs_alloc[bk];
                c_my = bs_chunk_of(a_my);
                if (c_my >= al_my && a_my == bs_chunk_start(c_my)) {
                    int32_t need = bs_chunk_cap(c_my);
                    int32_t base = atomicAdd(A.bs_pool_top, need);
                    if (base < 0 || base > A.bs_pool_cap - need) status = ST_LOG_OVERFLOW;
                    else { A.bs_dir[(int64_t)bk * BDIR + c_my] = base; if (bk == s_dirb) s_dir[c_my] = base; }
                }
            }
            // the push ids of this round start at G.push_cnt: read BEFORE the barrier -- thread 0 advances the counter behind it, and a wave
            // that came out of the barrier late used to read the advanced value (ids of two rounds overlapped: a wrong LIFO order inside a
            // bucket, once in some thousand batched calls -- the "graph 851" mismatch of round 2)
            const int32_t id0 = G.push_cnt;
            if (__syncthreads_or(status != 0)) { if (tid == 0) s_status = ST_LOG_OVERFLOW; BSYNC(); break; }
            if (S.jitter > 0 && ((threadIdx.x >> 6) & 1)) for (int _q = 0; _q < S.jitter; ++_q) __builtin_amdgcn_s_sleep(8);
            if (mine) {
                int32_t sl = A.bs_dir[(int64_t)bk * BDIR + c_my] + (a_my - bs_chunk_start(c_my));
                A.bs_v[sl] = x_my; A.bs_id[sl] = id0 + pos_my;
                A.vr[x_my].pqpos = id0 + pos_my;
                if (tail_my) {   // last move of its bucket group: the stack's new height (and chunk count)
                    A.bs_cnt[bk] = a_my + 1;
                    if (c_my + 1 > al_my) A.bs_alloc[bk] = c_my + 1;
                }
            }
            if (tid == 0) {
                if ((int32_t)bmin < G.minlist) G.minlist = (int32_t)bmin;
                G.push_cnt = id0 + nmoves;
            }
        }
        PHASE_STAMP(8);
        // ---- round epilogue ----
        if (tid < nc) batch_pos[L.cand[tid].v] = -1;
        if (tid == 0) {
            G.n_draws = L.cand[P - 1].draw0 + L.cand[P - 1].ndraw;   // offsets are a running sum (P2)
            s_nc = 0; s_pmax = BATCH + 1; s_p = BATCH + 1; s_ncont = 0; s_nmoves = 0; s_anydep = 0; s_npatched = 0;
        }
        done += P;
        pending_long = (OV == OV_RANDOM) && P < nc && (L.cand[P].flags & CF_BIG) != 0;
        BSYNC();
    }
    BSYNC();
    if (tid == 0) {
        G.n_elim = (int32_t)(handover ? done : nelim);
        if (s_status) G.status = s_status;
        G.pad0 = rounds; G.pad1 = singles;
        G.pool_cur = s_pool_cur; G.pool_end = s_pool_end;
        if constexpr (NARROW) {
            // the 32-slot kernel that follows on the stream continues from n_elim: at once after a hand-over, with nothing to do otherwise
            G.resume = 1;
            if (handover) G.narrow = 1;
            G.narrow_rounds += rounds - rounds_in;
        }
        if (S.prof && g == 0) {   // (the 16-slot kernel's sums go to a block of their own behind the other's; counts: this launch's)
            long long* const pr = S.prof + (NARROW ? 40 : 0);
            for (int q = 0; q < 20; ++q) pr[q] = s_prof[q];
            pr[20] = clock64() - clk0; pr[21] = wall_clock64() - wall0; pr[22] = rounds - rounds_in; pr[23] = singles - singles_in;
            for (int q = 24; q < 40; ++q) pr[q] = s_prof[q];
        }
        gd[g] = G;
    }
}
#undef BSYNC

#ifndef RLAP_ELIM_PQ_TU
// The handle's tables of std::sort's permutation of 17..BC all-equal keys (layout: rlap_kernels.h EQTAB_*), built once.
template <int BC>
__global__ __launch_bounds__(64) void k_eq_tables(uint8_t* __restrict__ out) {
    __shared__ CandT<BC> c[16];
    const int tid = threadIdx.x;
    Arrays A = {};
    A.o_v = OV_RANDOM; A.o_n = ON_ASC;   // all keys equal: asc and desc compare alike
    for (int base = 0; base < BC - 16; base += 16) {
        const int row = base + tid;
        if (tid < 16 && row < BC - 16) {
            CandT<BC>& C = c[tid];
            const int nn = 17 + row;
            for (int q = 0; q < nn; ++q) { C.e[q].aux = 1.0; C.ksel[q] = (uint8_t)q; }
            C.m = nn;
            cand_order_index_call(A, C);
            uint8_t* perm = out + row * BC;
            uint8_t* inv = out + (BC - 16) * BC + row * BC;
            for (int q = 0; q < BC; ++q) perm[q] = q < nn ? C.ksel[q] : (uint8_t)q;
            for (int q = 0; q < BC; ++q) inv[perm[q]] = (uint8_t)q;
        }
        __syncthreads();
    }
}

void launch_eq_tables(hipStream_t stream, uint8_t* out) {
    hipLaunchKernelGGL(k_eq_tables<64>, dim3(1), dim3(64), 0, stream, out);
    hipLaunchKernelGGL(k_eq_tables<32>, dim3(1), dim3(64), 0, stream, out + EQTAB_OFF32);
    hipLaunchKernelGGL(k_eq_tables<128>, dim3(1), dim3(64), 0, stream, out + EQTAB_OFF128);
}

// the priority-queue instantiations live in the other translation unit (top of this file)
int launch_eliminate_pq(int o_v, int o_n, unsigned G, bool many, bool narrow, hipStream_t stream, const Arrays& A, GraphDesc* gd, const ElimScratch& S,
                        int32_t* batch_pos, const int32_t* flags, const double* acc, const SqueezeBufs* sq, Arrays* A_cur);

// more graphs than CUs: the 256-thread shape (launch_eliminate_batch)
static bool elim_shape_many(unsigned G, int n_cu) {
    if (n_cu <= 0) n_cu = 256;
    bool many = G > (unsigned)n_cu;
    if (const char* e = std::getenv("RLAP_BATCH_SHAPE")) { if (e[0] == '2') many = true; else if (e[0] == '1') many = false; }   // diagnostic override: 256 / 1024
    return many;
}
// degree order, 1024-thread shape: the 16-slot kernel runs first (launch_eliminate_pq)
static bool elim_narrow(int o_v, bool many) {
    bool narrow = o_v == OV_DEGREE && !many;
    if (const char* e = std::getenv("RLAP_NARROW")) { if (e[0] == '0') narrow = false; }   // diagnostic override: the 32-slot kernel alone
    return narrow;
}
int squeeze_passes(int o_v, unsigned G, int n_cu, bool depths, bool views, int64_t nnz_ub) {
    if (!elim_narrow(o_v, elim_shape_many(G, n_cu)) || depths || views) return 0;
    bool on = nnz_ub >= SQUEEZE_MIN_NNZ;
    if (const char* e = std::getenv("RLAP_SQUEEZE")) { if (e[0] == '0') on = false; else if (e[0] == '1') on = true; }   // diagnostic override of the size gate
    return on ? SQUEEZE_PASSES : 0;
}

int launch_eliminate_batch(int o_v, int o_n, unsigned G, int n_cu, hipStream_t stream, const Arrays& A, GraphDesc* gd, const ElimScratch& S,
                           int32_t* batch_pos, const int32_t* flags, const double* acc, bool wide, const SqueezeBufs* sq, Arrays* A_cur) {
    *A_cur = A;
    // o_v = random meets long columns all the time (19 % of BA(1M,10) have more than 32 live entries when their
    // turn comes): it runs with 64 slots per candidate (64 candidates per round); the min-degree orders with 32.
    // more graphs than CUs: the 256-thread shape, four workgroups per CU (128 VGPRs, 39 KB of LDS; measured on 4096-node graphs: the same
    // time per graph as the 1024-thread shape, which is only ahead when one graph offers more than 32 independent vertices a round)
    const bool many = elim_shape_many(G, n_cu);
    // o_v = random on graphs with long columns (`wide`, chosen by the caller from the entries per vertex): 128 slots per
    // candidate, 32 candidates per round -- a column of 65..128 entries no longer ends the round (BA(4096,8): 134 rounds + 13
    // single vertices instead of 148 + 60).  Sparse graphs fill their rounds with 64 slots and keep 64 candidates.
    if (const char* e = std::getenv("RLAP_WIDE")) { if (e[0] == '1') wide = true; else if (e[0] == '0') wide = false; }   // diagnostic override
    if (wide && !many && o_v == OV_RANDOM) {
        if (o_n == ON_ASC) hipLaunchKernelGGL((k_eliminate_batch_t<OV_RANDOM, ON_ASC, 128, 1024>), dim3(G), dim3(1024), 0, stream, A, gd, S, batch_pos, flags, acc);
        else if (o_n == ON_DESC) hipLaunchKernelGGL((k_eliminate_batch_t<OV_RANDOM, ON_DESC, 128, 1024>), dim3(G), dim3(1024), 0, stream, A, gd, S, batch_pos, flags, acc);
        else hipLaunchKernelGGL((k_eliminate_batch_t<OV_RANDOM, ON_RANDOM, 128, 1024>), dim3(G), dim3(1024), 0, stream, A, gd, S, batch_pos, flags, acc);
        return 0;
    }
#define RLAP_CASE(OV, ON, BC) if (o_v == OV && o_n == ON) { \
        if (many) hipLaunchKernelGGL((k_eliminate_batch_t<OV, ON, BC, 256>), dim3(G), dim3(256), 0, stream, A, gd, S, batch_pos, flags, acc); \
        else hipLaunchKernelGGL((k_eliminate_batch_t<OV, ON, BC, 1024>), dim3(G), dim3(1024), 0, stream, A, gd, S, batch_pos, flags, acc); \
        return 0; }
    RLAP_CASE(OV_RANDOM, ON_ASC, 64) RLAP_CASE(OV_RANDOM, ON_DESC, 64) RLAP_CASE(OV_RANDOM, ON_RANDOM, 64)
#undef RLAP_CASE
    return launch_eliminate_pq(o_v, o_n, G, many, elim_narrow(o_v, many), stream, A, gd, S, batch_pos, flags, acc, sq, A_cur);
}
#else   // RLAP_ELIM_PQ_TU
constexpr int NARROW_BATCH_LATE = 144;   // candidates a round of the 16-slot kernel predicts behind a squeeze pass (NARROW_BATCH = 192 in front of the first); RLAP_NARROW_BATCH_LATE for measurements
int launch_eliminate_pq(int o_v, int o_n, unsigned G, bool many, bool narrow, hipStream_t stream, const Arrays& A_in, GraphDesc* gd, const ElimScratch& S,
                        int32_t* batch_pos, const int32_t* flags, const double* acc, const SqueezeBufs* sq, Arrays* A_cur) {
    // degree order, 1024-thread shape (`narrow`): the 16-slot kernel first (256 candidates per round while the columns at the head of
    // the queue are short: BA(1M,10) has none longer than 16 slots among its first 270,000 pops); it stops in front of the first longer
    // column and the 32-slot kernel below, launched right behind it, continues from there (GraphDesc::resume) -- or finds nothing left to do.
    // With squeeze passes (`sq`): a column's extent counts its dead entries, and for another 110,000 pops of that graph it is one to
    // four of those that make a column longer than 16 slots.  Each pass (rlap_squeeze.hip, all CUs) rewrites the surviving columns
    // into the other arena without them and clears GraphDesc::narrow, and the 16-slot kernel is launched again: it ends at once where
    // nothing is left to do or the first candidate is still too long.  All on the one stream; the host only keeps track of which arena
    // is current.  The hand-over behind the last pass is final.
    Arrays A = A_in;
    auto launch16 = [&](const ElimScratch& S16) {
        if (o_n == ON_ASC) hipLaunchKernelGGL((k_eliminate_batch_t<OV_DEGREE, ON_ASC, 16, 1024>), dim3(G), dim3(1024), 0, stream, A, gd, S16, batch_pos, flags, acc);
        else if (o_n == ON_DESC) hipLaunchKernelGGL((k_eliminate_batch_t<OV_DEGREE, ON_DESC, 16, 1024>), dim3(G), dim3(1024), 0, stream, A, gd, S16, batch_pos, flags, acc);
        else hipLaunchKernelGGL((k_eliminate_batch_t<OV_DEGREE, ON_RANDOM, 16, 1024>), dim3(G), dim3(1024), 0, stream, A, gd, S16, batch_pos, flags, acc);
    };
    // behind a squeeze the columns at the head of the queue hold 13 to 16 live entries, and the move list (1,024 moves a round) ends
    // a round at about 105 committed candidates: what is predicted beyond that is prepared, sampled and replayed for nothing
    ElimScratch S_late = S;
    S_late.narrow_batch = S.narrow_batch < NARROW_BATCH_LATE ? S.narrow_batch : NARROW_BATCH_LATE;
    if (const char* e = std::getenv("RLAP_NARROW_BATCH_LATE")) { const int q = std::atoi(e); S_late.narrow_batch = q < 1 ? 1 : (q > 256 ? 256 : q); }   // diagnostic override
    if (narrow) {
        launch16(S);
        for (int p = 0; sq && p < sq->passes; ++p) {
            // pass p reads the current arena and writes the other one: the call's first arena and sq->e2 take turns
            Slot* const e_dst = (p & 1) ? A_in.e : sq->e2;
            int32_t* const colptr_dst = (p & 1) ? const_cast<int32_t*>(A_in.colptr) : sq->colptr2;
            const int rc = launch_squeeze(stream, A, *sq, p, e_dst, colptr_dst, gd, (int32_t)G, flags, acc);
            if (rc) return rc;
            A.e = e_dst; A.colptr = colptr_dst;
            launch16(S_late);
        }
    }
    *A_cur = A;
#define RLAP_CASE(OV, ON, BC) if (o_v == OV && o_n == ON) { \
        if (many) hipLaunchKernelGGL((k_eliminate_batch_t<OV, ON, BC, 256>), dim3(G), dim3(256), 0, stream, A, gd, S, batch_pos, flags, acc); \
        else hipLaunchKernelGGL((k_eliminate_batch_t<OV, ON, BC, 1024>), dim3(G), dim3(1024), 0, stream, A, gd, S, batch_pos, flags, acc); \
        return 0; }
    RLAP_CASE(OV_DEGREE, ON_ASC, 32) RLAP_CASE(OV_DEGREE, ON_DESC, 32) RLAP_CASE(OV_DEGREE, ON_RANDOM, 32)
    RLAP_CASE(OV_COARSEN, ON_ASC, 32) RLAP_CASE(OV_COARSEN, ON_DESC, 32) RLAP_CASE(OV_COARSEN, ON_RANDOM, 32)
#undef RLAP_CASE
    return 0;
}
#endif  // RLAP_ELIM_PQ_TU

}  // namespace rlap
