// The degree order's squeeze schedule on the CPU (tests/test_squeeze_mirror.py): the round structure of host_mirror.cc's batch
// driver for the degree order with CandT<16> (host_mirror.cc itself is left as it is: the rounds are restated below without its
// statistics and without the coarsening branch) and, where the device's 16-slot kernel hands over (the first candidate of a round
// has more than 16 slots), the squeeze of rlap_core.h -- squeeze_rank_col, a prefix sum, squeeze_entry: the statements
// rlap_squeeze.hip runs -- into a second arena, then 16-slot rounds again.  After SQUEEZE_PASSES squeezes a long first candidate takes
// the single-vertex path (the device launches the 32-slot kernel there).  Every squeeze is checked on the spot; what fails is
// counted in the statistics.
#include "host_mirror.cc"

namespace {

struct SqueezeHook {
    int passes = 0, progress = 0;
    int64_t bad_twin = 0, bad_order = 0, bad_pool = 0, bad_entry = 0;
    int64_t at[SQUEEZE_PASSES] = {};            // vertices eliminated when pass p ran
    int64_t final_at = -1;                      // ... and at the hand-over behind the last pass (-1: none)
    std::vector<Slot> e2;
    std::vector<int32_t> colptr2, rank, cnt;

    // the first candidate of a round is longer than the record.  true: the columns were squeezed and the round is predicted again
    bool first_is_big(Setup& S, int64_t done) {
        if (passes >= SQUEEZE_PASSES) { if (final_at < 0) final_at = done; return false; }   // the last hand-over is final
        if (passes > 0 && done > at[passes - 1]) ++progress;
        at[passes++] = done;
        const Arrays& A = S.A;
        const int32_t N = (int32_t)S.n;
        // what every surviving column shows a traversal, before
        std::vector<std::vector<std::pair<int32_t, double>>> before((size_t)N);
        for (int32_t v = 0; v < N; ++v) if (A.vr[v].pqpos != -2)
            col_for_each_slot(A, v, [&](int32_t s) { if (A.e[s].val > 0) before[v].push_back({A.e[s].nbr, A.e[s].val}); });
        // ---- the pass: rank, scan, copy, epilogue ----
        rank.assign((size_t)A.slot_cap, -1); cnt.assign((size_t)N + 1, 0); colptr2.assign((size_t)N + 1, 0);
        e2.assign((size_t)A.slot_cap, Slot{0.0, 0, -1});
        for (int32_t v = 0; v < N; ++v) cnt[v] = A.vr[v].pqpos != -2 ? squeeze_rank_col(A, v, rank.data()) : 0;
        for (int32_t v = 0; v < N; ++v) colptr2[v + 1] = colptr2[v] + cnt[v];
        for (int32_t v = 0; v < N; ++v) if (colptr2[v + 1] != colptr2[v])
            col_for_each_slot(A, v, [&](int32_t s) { if (A.e[s].val > 0 && !squeeze_entry(A, rank.data(), colptr2.data(), e2.data(), N, v, s)) ++bad_entry; });
        for (int32_t v = 0; v < N; ++v) { A.vr[v].app_cnt = 0; A.vr[v].app_chunk = -1; }
        S.ent.swap(e2); S.colptr.swap(colptr2);
        S.A.e = S.ent.data(); S.A.colptr = S.colptr.data();
        S.pool_top = S.colptr[N];
        S.G.pool_cur = 0; S.G.pool_end = 0; S.G.narrow = 0;
        // ---- checks ----
        if (*A.pool_top != A.colptr[N]) ++bad_pool;
        for (int32_t v = 0; v < N; ++v) {
            for (int32_t s = A.colptr[v]; s < A.colptr[v + 1]; ++s) {
                const Slot& x = A.e[s];
                if (!(x.val > 0) || x.twin < 0 || x.twin >= A.colptr[N] || A.e[x.twin].twin != s || A.e[x.twin].nbr != v ||
                    x.twin < A.colptr[x.nbr] || x.twin >= A.colptr[x.nbr + 1]) ++bad_twin;
            }
            std::vector<std::pair<int32_t, double>> after;
            if (A.vr[v].pqpos != -2) col_for_each_slot(A, v, [&](int32_t s) { if (A.e[s].val > 0) after.push_back({A.e[s].nbr, A.e[s].val}); });
            if (after != before[v]) ++bad_order;
        }
        return true;
    }
};

// 16-slot rounds of the degree order (host_mirror.cc::mirror_batch_impl<16> with o_v = degree): predict, prepare, dependence, patch +
// sample, PQ replay with contended targets in candidate order, commit of the longest prefix no move pre-empts.
// stats[0] = rounds, [1] = single vertices.
int squeeze_rounds(Setup& S, int32_t Bsz, SqueezeHook& H, int64_t nelim, int64_t* order_out, int64_t* npop_out, int64_t* stats) {
    constexpr int BC = 16;
    typedef CandT<BC> Cand;
    const Arrays& A = S.A;
    GraphDesc& G = S.G;
    const int64_t n = S.n;
    int64_t done = 0, npop = 0, rounds = 0, singles = 0;
    std::vector<Cand> cand((size_t)Bsz);
    std::vector<int32_t> batch_pos((size_t)n, -1), tcount((size_t)n, 0);
    struct CRec { int32_t x, i, j; };
    struct Move { uint64_t key; int32_t v; };
    while (done < nelim) {
        ++rounds;
        const int32_t Bcur = (int32_t)std::min<int64_t>(Bsz, nelim - done);
        // ---- P0: predict the next pops ----
        int32_t nc = 0, b = 0;
        while (true) {
            b = G.bucket_base + G.minlist;
            for (int32_t a = A.bs_cnt[b] - 1; a >= 0 && nc < Bcur; --a) {
                const int32_t s = bs_slot(A, b, a), v = A.bs_v[s];
                if (A.vr[v].pqpos == A.bs_id[s]) { cand[nc].v = v; cand[nc].src = a; ++nc; }
            }
            for (int32_t oc = A.ocur[b]; oc < A.oend[b] && nc < Bcur; ++oc) {
                const int32_t v = A.orig_order[oc];
                if (A.vr[v].pqpos == -1) { cand[nc].v = v; cand[nc].src = ~oc; ++nc; }
            }
            if (nc > 0) break;
            A.bs_cnt[b] = 0; A.ocur[b] = A.oend[b];
            G.minlist += 1;
            if (G.minlist > 2 * G.n) return ST_INTERNAL;
        }
        // ---- P1: prepare; the hand-over ----
        for (int32_t i = 0; i < nc; ++i) { const int32_t v = cand[i].v, src = cand[i].src; cand_prepare(A, v, cand[i]); cand[i].src = src; }
        if ((cand[0].flags & CF_BIG) && H.first_is_big(S, done)) { --rounds; continue; }   // nothing popped, nothing marked: predicted again
        for (int32_t i = 0; i < nc; ++i) batch_pos[cand[i].v] = i;
        // ---- P1b: dependence; Pmax ----
        int32_t Pmax = nc;
        for (int32_t i = 0; i < nc; ++i) {
            Cand& C = cand[i];
            bool bad = (C.flags & (CF_BIG | CF_DUP)) != 0;
            C.ndep = 0;
            if (!bad) for (int32_t j = 0; j < C.m; ++j) {
                const int32_t bp = batch_pos[C.e[j].nbr];
                if (bp >= 0 && bp < i) { if (C.ndep >= DEPMAX) { bad = true; break; } C.dep[C.ndep++] = (uint8_t)bp; }
            }
            if (bad && i < Pmax) Pmax = i;
        }
        auto consume = [&](int32_t P) {   // candidates [0,P) leave the queue
            const int32_t src = cand[P - 1].src;
            if (src >= 0) A.bs_cnt[b] = src; else { A.bs_cnt[b] = 0; A.ocur[b] = (~src) + 1; }
            for (int32_t i = 0; i < P; ++i) A.vr[cand[i].v].pqpos = -2;
        };
        auto cleanup = [&]() { for (int32_t i = 0; i < nc; ++i) batch_pos[cand[i].v] = -1; };
        auto single = [&]() -> int {      // candidate 0 takes the single-vertex path
            ++singles;
            consume(1);
            cleanup();
            if (order_out) order_out[npop] = cand[0].v;
            ++npop;
            const int rc = serial_eliminate(A, G, S.B, S.cap, cand[0].v, done + 1);
            done += 1;
            return rc;
        };
        if (Pmax == 0) { const int rc = single(); if (rc) return rc; continue; }
        // ---- P2: RNG offsets; P3: sampling, dependent candidates patched first ----
        int64_t off = G.n_draws;
        for (int32_t i = 0; i < Pmax; ++i) { cand[i].draw0 = off; off += cand[i].ndraw; }
        if (off > A.rng_len) return ST_RNG_OVERFLOW;
        for (int32_t i = 0; i < Pmax; ++i) {
            if (cand[i].ndep > 0 && !cand_patch(A, cand.data(), i, G.vbase)) { Pmax = i; break; }
            cand_sample(A, cand[i]);
        }
        // ---- P4: PQ replay with contended targets in candidate order ----
        for (int32_t i = 0; i < Pmax; ++i) for (int32_t j = 0; j < cand[i].m; ++j) tcount[cand[i].e[j].nbr]++;
        std::vector<CRec> cont;
        for (int32_t i = 0; i < Pmax; ++i) {
            Cand& C = cand[i];
            const bool allow_last = (done + i + 1) + 1 < n;
            for (int32_t j = 0; j < C.m; ++j) {
                const int32_t x = C.e[j].nbr;
                TRes& R = ent_tres(C.e[j]);
                if (tcount[x] > 1) { R.flags = TF_CONTENDED; cont.push_back({x, i, j}); continue; }
                int mv, c; bool cx = false;
                const int32_t k2 = cand_replay(A, C, j, A.vr[x].key, G.n, allow_last, &mv, &c, &cx);
                R.key_after = k2; R.mv = (int16_t)mv; R.c = (uint8_t)c; R.flags = 0;
                if (cx) C.flags |= CF_COMPLEX;
            }
        }
        std::sort(cont.begin(), cont.end(), [](const CRec& p, const CRec& q) { return p.x != q.x ? p.x < q.x : p.i < q.i; });
        for (size_t q = 0; q < cont.size();) {
            size_t r = q;
            int32_t key = A.vr[cont[q].x].key;
            while (r < cont.size() && cont[r].x == cont[q].x) {
                Cand& C = cand[cont[r].i];
                const bool allow_last = (done + cont[r].i + 1) + 1 < n;
                int mv, c; bool cx = false;
                const int32_t k2 = cand_replay(A, C, cont[r].j, key, G.n, allow_last, &mv, &c, &cx);
                TRes& R = ent_tres(C.e[cont[r].j]);
                R.key_after = k2; R.mv = (int16_t)mv; R.c = (uint8_t)c;
                if (cx) C.flags |= CF_COMPLEX;
                key = k2;
                ++r;
            }
            q = r;
        }
        // ---- P: first pre-emption / complex candidate ----
        int32_t P = Pmax;
        for (int32_t i = 0; i < Pmax; ++i) {
            Cand& C = cand[i];
            if (C.flags & CF_COMPLEX) { P = std::min(P, i); break; }
            bool pre = false;
            for (int32_t j = 0; j < C.m; ++j) { TRes& R = ent_tres(C.e[j]); if (R.mv >= 0 && pq_list_of(R.key_after, G.n) <= G.minlist) pre = true; }
            if (pre) { P = std::min(P, i + 1); break; }
        }
        for (int32_t i = 0; i < Pmax; ++i) for (int32_t j = 0; j < cand[i].m; ++j) tcount[cand[i].e[j].nbr] = 0;
        if (P == 0) { const int rc = single(); if (rc) return rc; continue; }
        // ---- P5: commit candidates [0,P) ----
        consume(P);
        for (int32_t i = 0; i < P; ++i) { if (order_out) order_out[npop] = cand[i].v; ++npop; }
        std::vector<Move> moves;
        std::vector<CRec> all;
        for (int32_t i = 0; i < P; ++i) for (int32_t j = 0; j < cand[i].m; ++j) all.push_back({cand[i].e[j].nbr, i, j});
        std::sort(all.begin(), all.end(), [](const CRec& p, const CRec& q) { return p.x != q.x ? p.x < q.x : p.i < q.i; });
        std::vector<std::vector<int32_t>> pslot((size_t)P, std::vector<int32_t>(BC, -1));   // slots of the pushes, by (candidate, position)
        for (size_t q = 0; q < all.size(); ++q) {
            Cand& C = cand[all[q].i];
            const int32_t x = all[q].x, j = all[q].j;
            const TRes R = ent_tres(C.e[j]);
            for (int32_t p = 0; p < C.m - 1; ++p) if (C.ksel[p] == j) { const int32_t s = col_append(A, x); if (s < 0) return ST_POOL_OVERFLOW; pslot[all[q].i][p] = s; }
            const bool last_of_x = (q + 1 == all.size()) || all[q + 1].x != x;
            if (last_of_x) {   // final state of x after the committed prefix; its last move may stem from an earlier record
                int32_t mvseq = -1;
                for (size_t r = q + 1; r-- > 0 && all[r].x == x;) {
                    const TRes Rr = ent_tres(cand[all[r].i].e[all[r].j]);
                    if (Rr.mv >= 0) { mvseq = (all[r].i << 8) | Rr.mv; break; }
                }
                if (R.key_after != A.vr[x].key) A.vr[x].key = R.key_after;
                if (mvseq >= 0) moves.push_back({((uint64_t)(uint32_t)pq_list_of(R.key_after, G.n) << 32) | (uint32_t)mvseq, x});
            }
        }
        for (int32_t i = 0; i < P; ++i) {   // rewires + kills
            Cand& C = cand[i];
            const int32_t m = C.m;
            for (int32_t j = 0; j < m - 1; ++j) {
                const int32_t k = C.e[C.ksel[j]].nbr, s_n = pslot[i][j];
                int32_t s_r = C.e[j].twin;
                if (s_r < 0) s_r = pslot[(~s_r) / BC][(~s_r) % BC];   // patched entry: the slot an earlier candidate of this round appends
                const double nw = C.e[j].val;
                A.e[s_r].nbr = k; A.e[s_r].val = nw; A.e[s_r].twin = s_n;
                A.e[s_n].nbr = C.e[j].nbr; A.e[s_n].val = nw; A.e[s_n].twin = s_r;
            }
            if (m >= 1) { int32_t s_l = C.e[m - 1].twin; if (s_l < 0) s_l = pslot[(~s_l) / BC][(~s_l) % BC]; A.e[s_l].val = 0; }
            G.n_draws += C.ndraw;
        }
        std::sort(moves.begin(), moves.end(), [](const Move& p, const Move& q) { return p.key < q.key; });
        for (const Move& mvv : moves) { const int rc = pq_push(A, G, mvv.v, (int32_t)(mvv.key >> 32)); if (rc) return rc; }
        cleanup();
        done += P;
    }
    stats[0] = rounds; stats[1] = singles;
    *npop_out = npop;
    return 0;
}


}  // namespace

// stats_out: [0] rounds, [1] single vertices, [20] squeezes run, [21] squeezes after which a 16-slot round committed, [22..25]
// failed checks (twin links, traversal order, pool top, entries out of range), [26], [27] vertices eliminated when each squeeze ran
extern "C" int mirror_approx_chol_batch_squeeze(const int64_t* row, const int64_t* col, const double* w, int64_t E, int64_t n, int64_t t,
                                                int o_v, int o_n, const int64_t* perm, uint64_t shuffle_seed, int32_t pool_slots, int32_t Bsz,
                                                double** out, int64_t* out_rows, int64_t* order_out, int64_t* stats_out) {
    if (o_v != OV_DEGREE) return ST_BAD_ARG;
    Setup S;
    S.build(row, col, w, E, n, t, o_v, o_n, perm, shuffle_seed, pool_slots);
    int64_t nelim = std::min<int64_t>(t, n - 1);
    if (nelim < 0) nelim = 0;
    SqueezeHook H;
    int64_t npop = 0;
    const int rc = squeeze_rounds(S, Bsz, H, nelim, order_out, &npop, stats_out);
    if (rc) return rc;
    if (H.passes > 0 && (H.final_at >= 0 ? H.final_at : nelim) > H.at[H.passes - 1]) ++H.progress;   // (16-slot rounds behind the last squeeze)
    stats_out[20] = H.passes; stats_out[21] = H.progress;
    stats_out[22] = H.bad_twin; stats_out[23] = H.bad_order; stats_out[24] = H.bad_pool; stats_out[25] = H.bad_entry;
    for (int p = 0; p < SQUEEZE_PASSES && p < 2; ++p) stats_out[26 + p] = H.at[p];
    return S.finish(nelim, npop, order_out, out, out_rows);
}
