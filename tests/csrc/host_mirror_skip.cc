// The degree order's rounds with the replay restricted to the pairs an elimination touches (tests/test_skip_mirror.py): the round
// structure of host_mirror.cc's batch driver for the degree order (host_mirror.cc itself is left as it is; the rounds are restated
// below as host_mirror_squeeze.cc restates them), with CandT<16> and CandT<32> records, where the target counts, the contended list,
// the replay and the commit see only the (candidate, target) pairs rlap_core.h::cand_touches passes -- the predicate the round
// kernel calls.  An untouched pair's record reads c = 0, mv = -1, as the kernel writes it.  Neither driver has a move cap or a
// record cap.  Beside the rows and the pop order the drivers count what the rule removes.
#include "host_mirror.cc"

namespace {

// stats[0] rounds, [1] single vertices, [2] rounds of the 16-slot driver, [3] (candidate, target) pairs of the sampled candidates,
// [4] those the rule passes, [5] contended records without the rule, [6] with it, [7] candidates flagged complex (keys beyond n) with
// the rule, [8] without it, [9] vertices eliminated at the hand-over (-1: none)
// stop_on_big: a first candidate longer than the record ends the driver (the hand-over to the 32-slot rounds)
template <int BC>
int skip_rounds(Setup& S, int32_t Bsz, bool stop_on_big, int64_t nelim, int64_t& done, int64_t& npop, int64_t* order_out, int64_t* stats) {
    typedef CandT<BC> Cand;
    const Arrays& A = S.A;
    GraphDesc& G = S.G;
    const int64_t n = S.n;
    std::vector<Cand> cand((size_t)Bsz);
    std::vector<int32_t> batch_pos((size_t)n, -1), tcount((size_t)n, 0), tcount_all((size_t)n, 0);
    struct CRec { int32_t x, i, j; };
    struct Move { uint64_t key; int32_t v; };
    while (done < nelim) {
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
        if (stop_on_big && (cand[0].flags & CF_BIG)) return 0;   // nothing popped, nothing marked: the 32-slot rounds predict again
        ++stats[0];
        if (BC == 16) ++stats[2];
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
            ++stats[1];
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
        std::vector<char> would_cx((size_t)Pmax, 0);
        // ---- P4.1: the key-independent half of the replay, parked in the pair's record; only touched pairs are counted ----
        for (int32_t i = 0; i < Pmax; ++i) {
            Cand& C = cand[i];
            for (int32_t j = 0; j < C.m; ++j) {
                int c0, li0;
                cand_replay_pre(A, C, j, &c0, &li0);
                TRes& R = ent_tres(C.e[j]);
                const int32_t x = C.e[j].nbr;
                ++stats[3];
                tcount_all[x]++;
                R.key_after = 0; R.flags = 0;
                if (!cand_touches(A.o_v, C.m, j, C.koff, c0)) {
                    R.c = 0; R.mv = -1;
                    if (A.vr[x].key > G.n) would_cx[i] = 1;   // (statistics only: the complex test fired on this pair -- judged by the key before the round)
                    continue;
                }
                R.c = (uint8_t)c0; R.mv = (int16_t)li0;
                ++stats[4];
                tcount[x]++;
            }
        }
        for (int32_t i = 0; i < Pmax; ++i) for (int32_t j = 0; j < cand[i].m; ++j) if (tcount_all[cand[i].e[j].nbr] > 1) ++stats[5];
        // ---- P4.2: replay; contended targets in candidate order ----
        auto touched = [&](const Cand& C, int32_t j) { return cand_touches(A.o_v, C.m, j, C.koff, (int)C.e[j].res.c); };
        std::vector<CRec> cont;
        for (int32_t i = 0; i < Pmax; ++i) {
            Cand& C = cand[i];
            const bool allow_last = (done + i + 1) + 1 < n;
            for (int32_t j = 0; j < C.m; ++j) {
                if (!touched(C, j)) continue;
                const int32_t x = C.e[j].nbr;
                TRes& R = ent_tres(C.e[j]);
                if (tcount[x] > 1) { R.flags = TF_CONTENDED; cont.push_back({x, i, j}); continue; }
                int mv; bool cx = false;
                const int32_t k2 = cand_replay_post(A, C, j, A.vr[x].key, G.n, allow_last, (int)R.c, (int)R.mv, &mv, &cx);
                R.key_after = k2; R.mv = (int16_t)mv;
                if (cx) C.flags |= CF_COMPLEX;
            }
        }
        stats[6] += (int64_t)cont.size();
        std::sort(cont.begin(), cont.end(), [](const CRec& p, const CRec& q) { return p.x != q.x ? p.x < q.x : p.i < q.i; });
        for (size_t q = 0; q < cont.size();) {
            size_t r = q;
            int32_t key = A.vr[cont[q].x].key;
            while (r < cont.size() && cont[r].x == cont[q].x) {
                Cand& C = cand[cont[r].i];
                const bool allow_last = (done + cont[r].i + 1) + 1 < n;
                TRes& R = ent_tres(C.e[cont[r].j]);
                int mv; bool cx = false;
                const int32_t k2 = cand_replay_post(A, C, cont[r].j, key, G.n, allow_last, (int)R.c, (int)R.mv, &mv, &cx);
                R.key_after = k2; R.mv = (int16_t)mv;
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
            if (C.flags & CF_COMPLEX) ++stats[7];
            if ((C.flags & CF_COMPLEX) || would_cx[i]) ++stats[8];
        }
        for (int32_t i = 0; i < Pmax; ++i) {
            Cand& C = cand[i];
            if (C.flags & CF_COMPLEX) { P = std::min(P, i); break; }
            bool pre = false;
            for (int32_t j = 0; j < C.m; ++j) { TRes& R = ent_tres(C.e[j]); if (R.mv >= 0 && pq_list_of(R.key_after, G.n) <= G.minlist) pre = true; }
            if (pre) { P = std::min(P, i + 1); break; }
        }
        for (int32_t i = 0; i < Pmax; ++i) for (int32_t j = 0; j < cand[i].m; ++j) { tcount[cand[i].e[j].nbr] = 0; tcount_all[cand[i].e[j].nbr] = 0; }
        if (P == 0) { const int rc = single(); if (rc) return rc; continue; }
        // ---- P5: commit candidates [0,P): touched pairs only -- an untouched pair pushes nothing and moves nothing ----
        consume(P);
        for (int32_t i = 0; i < P; ++i) { if (order_out) order_out[npop] = cand[i].v; ++npop; }
        std::vector<Move> moves;
        std::vector<CRec> all;
        for (int32_t i = 0; i < P; ++i) for (int32_t j = 0; j < cand[i].m; ++j) if (touched(cand[i], j)) all.push_back({cand[i].e[j].nbr, i, j});
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
    return 0;
}

}  // namespace

// bc = 16: 16-slot rounds of Bsz candidates up to the first column of more than 16 slots at the head of the queue, then 32-slot rounds
// of Bsz32 candidates; bc = 32: 32-slot rounds of Bsz32 candidates alone.  stats_out: see skip_rounds.
extern "C" int mirror_approx_chol_batch_skip(const int64_t* row, const int64_t* col, const double* w, int64_t E, int64_t n, int64_t t,
                                             int o_v, int o_n, const int64_t* perm, uint64_t shuffle_seed, int32_t pool_slots, int bc,
                                             int32_t Bsz, int32_t Bsz32, double** out, int64_t* out_rows, int64_t* order_out, int64_t* stats_out) {
    if (o_v != OV_DEGREE || (bc != 16 && bc != 32)) return ST_BAD_ARG;
    Setup S;
    S.build(row, col, w, E, n, t, o_v, o_n, perm, shuffle_seed, pool_slots);
    int64_t nelim = std::min<int64_t>(t, n - 1);
    if (nelim < 0) nelim = 0;
    int64_t done = 0, npop = 0;
    for (int q = 0; q < 16; ++q) stats_out[q] = 0;
    stats_out[9] = -1;
    if (bc == 16) {
        const int rc = skip_rounds<16>(S, Bsz, true, nelim, done, npop, order_out, stats_out);
        if (rc) return rc;
        if (done < nelim) stats_out[9] = done;
    }
    const int rc = skip_rounds<32>(S, Bsz32, false, nelim, done, npop, order_out, stats_out);
    if (rc) return rc;
    return S.finish(nelim, npop, order_out, out, out_rows);
}
