// Host mirror of an edge plan (rlap_edge_plan_build): a whole plan built on the host from (rows, ptr, node_ptr, flags,
// fill) with the very headers rlap_edgeplan.hip includes -- rlap_edgeplan.h (the degree rule), rlap_gcnmath.h (the coefficients),
// rlap_plan.h (the layout) and rlap_spmm.h (the chunks) -- compiled with g++ -ffp-contract=off.  tests/test_edge_plan_cpu.py checks it
// against a numpy restatement of the rule, against tests/csrc/plan_mirror.cc on elimination results and against a plain Python
// construction; the GPU tests compare the device's buffer with it bit for bit.
// With -DEDGEPLAN_MIRROR_MAIN the file is a stand-alone program that builds the plans of hand-made inputs, checks them against
// lists built the plain way, and feeds two malformed inputs (an id out of range, a ptr past m) that must be refused: it is what
// runs under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "rlap_edgeplan.h"
#include "rlap_gcnmath.h"
#include "rlap_plan.h"
#include "rlap_spmm.h"

using namespace rlap;

namespace {

constexpr int WEIGHTED = 1, SELF_LOOPS = 2, NORMALIZE = 4;   // RLAP_GCN_* (include/rlap_hip.h)
constexpr int E_INDEX_RANGE = 2, E_BAD_ARG = 3;              // RLAP_E_*

bool table_ok(const int64_t* t, int64_t n, int64_t last) {
    if (t[0] != 0 || t[n] != last) return false;
    for (int64_t k = 0; k < n; ++k)
        if (t[k + 1] < t[k]) return false;
    return true;
}

bool id_ok(double v, int64_t lo, int64_t hi) { return v >= (double)lo && v < (double)hi && v == (double)(int64_t)v; }

}  // namespace

extern "C" {

int edgeplan_lanes() { return edgeplan::LANES; }
int edgeplan_accs() { return edgeplan::ACCS; }
unsigned edgeplan_key_bits(int64_t slots) { return edgeplan::key_bits(slots); }
// place_of inverts (lane_of, acc_of) on [0, n)
int edgeplan_places_consistent(int64_t n) {
    for (int64_t k = 0; k < n; ++k) {
        const int64_t turn = k / (edgeplan::LANES * edgeplan::ACCS);
        if (edgeplan::place_of(turn, edgeplan::acc_of(k), edgeplan::lane_of(k)) != k) return 0;
    }
    return 1;
}

// One direction of the plan of sc (m, 3) rows [source, target, w] in any order within the S segments of ptr; node_ptr [G + 1] or
// null (then G = 1); L = S / G layers of N ids; flags RLAP_GCN_*.  Writes deg, dis, lw, loopc [L N each] (loopc only with self
// loops), off[L N + 1], the records (rec_c, rec_id: m each at most) and the directory (dir_slot, dir_k: dir_cap(m) each at most),
// *chunks the directory entries, *loops_removed the loop rows that left.  Returns the records, or -RLAP_E_* for a refused input
// (then nothing else is written).
int64_t edgeplan_build(int64_t m, const double* sc, int64_t S, const int64_t* ptr, int64_t G, const int64_t* node_ptr, int64_t N, int flags,
                       double fill, int transpose, double* deg, double* dis, double* lw, double* loopc, int64_t* off, double* rec_c,
                       int32_t* rec_id, int64_t* dir_slot, int64_t* dir_k, int64_t* chunks, int64_t* loops_removed) {
    const bool weighted = (flags & WEIGHTED) != 0, loops = (flags & SELF_LOOPS) != 0, normalize = (flags & NORMALIZE) != 0;
    if (!node_ptr) G = 1;
    if (S < 1 || G < 1 || S % G != 0 || m < 0 || N < 0) return -E_BAD_ARG;
    if (!table_ok(ptr, S, m) || (node_ptr && !table_ok(node_ptr, G, N))) return -E_BAD_ARG;
    const int64_t slots = (S / G) * N;
    // the key pass: segment, ids, weight; the target and the source slot of every row
    std::vector<int64_t> key[2] = {std::vector<int64_t>((size_t)m), std::vector<int64_t>((size_t)m)};
    bool bad_id = false, bad_w = false;
    int64_t nloops = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t layer = s / G, g = s % G, lo = node_ptr ? node_ptr[g] : 0, hi = node_ptr ? node_ptr[g + 1] : N;
        for (int64_t r = ptr[s]; r < ptr[s + 1]; ++r) {
            const double vi = sc[3 * r], vj = sc[3 * r + 1];
            if (!id_ok(vi, lo, hi) || !id_ok(vj, lo, hi)) { bad_id = true; continue; }
            if (weighted && normalize && !gcnmath::weight_ok(sc[3 * r + 2])) bad_w = true;
            key[0][(size_t)r] = plan::slot_of(layer, N, (int64_t)vj);
            key[1][(size_t)r] = plan::slot_of(layer, N, (int64_t)vi);
            if (loops && vi == vj) ++nloops;
        }
    }
    if (bad_id) return -E_INDEX_RANGE;
    if (bad_w) return -E_BAD_ARG;
    auto weight = [&](int64_t r) { return weighted ? sc[3 * r + 2] : 1.0; };
    auto loop_row = [&](int64_t r) { return sc[3 * r] == sc[3 * r + 1]; };
    // the stable sorts and every slot's range
    std::vector<int64_t> perm[2], lo[2], hi[2];
    for (int d = 0; d < 2; ++d) {
        perm[d].resize((size_t)m);
        std::iota(perm[d].begin(), perm[d].end(), (int64_t)0);
        std::stable_sort(perm[d].begin(), perm[d].end(), [&](int64_t a, int64_t b) { return key[d][(size_t)a] < key[d][(size_t)b]; });
        lo[d].assign((size_t)slots, 0);
        hi[d].assign((size_t)slots, 0);
        for (int64_t p = 0; p < m; ++p) {
            const int64_t k = key[d][(size_t)perm[d][(size_t)p]];
            if (p == 0 || key[d][(size_t)perm[d][(size_t)p - 1]] != k) lo[d][(size_t)k] = p;
            hi[d][(size_t)k] = p + 1;
        }
    }
    // the degrees: the rule over the target's list
    for (int64_t slot = 0; slot < slots; ++slot) {
        const int64_t s0 = lo[0][(size_t)slot], n = hi[0][(size_t)slot] - s0;
        double w = fill;
        const double dg = edgeplan::degree(n, [&](int64_t k) { return weight(perm[0][(size_t)(s0 + k)]); },
                                           [&](int64_t k) { return loop_row(perm[0][(size_t)(s0 + k)]); }, loops, fill, &w);
        deg[slot] = dg;
        dis[slot] = gcnmath::dis(dg);
        lw[slot] = w;
        if (loops) loopc[slot] = normalize ? gcnmath::value(dis[slot], w, dis[slot]) : w;
    }
    // the lists of the direction, by rlap_plan.h's functions
    const int d = transpose ? 1 : 0;
    const bool drop = loops && nloops > 0;
    std::vector<int64_t> kept((size_t)slots + 1, 0);
    for (int64_t r = 0; r < m; ++r) kept[(size_t)key[d][(size_t)r]] += (drop && loop_row(r)) ? 0 : 1;
    off[0] = 0;
    for (int64_t s = 0; s < slots; ++s) off[s + 1] = off[s] + kept[(size_t)s];
    for (int64_t p = 0; p < m; ++p) {
        const int64_t r = perm[d][(size_t)p], slot = key[d][(size_t)r], f = lo[d][(size_t)slot];
        if (drop && loop_row(r)) continue;
        const int64_t place = drop ? plan::place_counting(p - f, [&](int64_t j) { return loop_row(perm[d][(size_t)(f + j)]); })
                                   : plan::place_plain(f, p);
        const int64_t at = plan::record_index(off[slot], off[slot + 1], place);
        if (at < 0 || at >= m) return -10;
        const double w = weight(r);
        rec_c[at] = normalize ? gcnmath::value(dis[key[1][(size_t)r]], w, dis[key[0][(size_t)r]]) : w;
        rec_id[at] = (int32_t)sc[3 * r + (transpose ? 1 : 0)];
    }
    int64_t q = 0;
    for (int64_t s = 0; s < slots; ++s) {
        plan::dir_write(s, kept[(size_t)s], q, plan::dir_cap(m), [&](int64_t at, plan::ChunkRef ref) { dir_slot[at] = ref.slot; dir_k[at] = ref.k; });
        q += plan::dir_chunks(kept[(size_t)s]);
    }
    *chunks = q;
    *loops_removed = loops ? nloops : 0;
    return off[slots];
}

}  // extern "C"

#ifdef EDGEPLAN_MIRROR_MAIN
#include <cstdio>

namespace {

struct Input { const char* name; std::vector<double> sc; std::vector<int64_t> ptr, node_ptr; int64_t N; int want; };

// num_nodes 9, six ids used: duplicates, three loop rows on id 2 with different weights, id 5 only a source, id 6 only a target, id
// 8 absent, an empty segment between two others
Input hand() {
    const double a[][3] = {{0, 1, 0.5}, {2, 2, 3.0}, {1, 0, 0.25}, {0, 1, 0.5}, {5, 0, 1.5}, {2, 2, 4.0}, {3, 6, 2.0}, {1, 2, 0.75},
                           {2, 2, 5.0}, {2, 1, 1.25}, {0, 3, 0.125}};
    const double b[][3] = {{3, 0, 1.0}, {0, 3, 2.0}, {5, 6, 0.5}, {1, 1, 9.0}};
    Input in{"hand", {}, {}, {}, 9, 0};
    for (auto& r : a) in.sc.insert(in.sc.end(), r, r + 3);
    for (auto& r : b) in.sc.insert(in.sc.end(), r, r + 3);
    in.ptr = {0, 11, 11, 15};
    return in;
}

Input star(int64_t leaves) {   // rows of the centre and of the leaves interleaved, two loop rows of the centre among them
    Input in{"star", {}, {}, {}, leaves + 1, 0};
    for (int64_t i = 0; i < leaves; ++i) {
        const double r0[3] = {0, (double)(i + 1), 0.5 + 0.001 * (double)i}, r1[3] = {(double)(i + 1), 0, 0.25 + 0.002 * (double)i};
        in.sc.insert(in.sc.end(), r0, r0 + 3);
        if (i == 7 || i == 400) { const double l[3] = {0, 0, 1.5 + (double)i}; in.sc.insert(in.sc.end(), l, l + 3); }
        in.sc.insert(in.sc.end(), r1, r1 + 3);
    }
    in.ptr = {0, (int64_t)in.sc.size() / 3};
    return in;
}

Input batch() {   // two graphs over ids [0, 3) and [3, 7), two layers
    const double rows[][3] = {{0, 1, 1.0}, {2, 1, 2.0}, {1, 0, 0.5}, {3, 6, 1.0}, {6, 3, 1.0}, {4, 4, 2.0}, {1, 2, 3.0}, {5, 3, 1.0}, {3, 5, 1.0}};
    Input in{"batch", {}, {}, {}, 7, 0};
    for (auto& r : rows) in.sc.insert(in.sc.end(), r, r + 3);
    in.ptr = {0, 3, 6, 7, 9};
    in.node_ptr = {0, 3, 7};
    return in;
}

int check(const Input& in, int flags, int transpose) {
    const int64_t m = (int64_t)in.sc.size() / 3, S = (int64_t)in.ptr.size() - 1, G = in.node_ptr.empty() ? 1 : (int64_t)in.node_ptr.size() - 1;
    const int64_t N = in.N, slots = (S / G) * N, cap = plan::dir_cap(m);
    std::vector<double> deg((size_t)slots), dis((size_t)slots), lw((size_t)slots), loopc((size_t)slots), rc((size_t)m);
    std::vector<int64_t> off((size_t)slots + 1), dslot((size_t)cap), dk((size_t)cap);
    std::vector<int32_t> rid((size_t)m);
    int64_t chunks = -1, removed = -1;
    const int64_t ent = edgeplan_build(m, in.sc.data(), S, in.ptr.data(), G, in.node_ptr.empty() ? nullptr : in.node_ptr.data(), N, flags, 2.0,
                                       transpose, deg.data(), dis.data(), lw.data(), loopc.data(), off.data(), rc.data(), rid.data(),
                                       dslot.data(), dk.data(), &chunks, &removed);
    if (in.want) return ent == -in.want ? 0 : 100;
    if (ent < 0) return 101;
    // the plain way: every list by appending in input order; the degrees by the same rule over it
    const bool loops = (flags & SELF_LOOPS) != 0;
    bool any = false;
    for (int64_t r = 0; r < m; ++r) any = any || in.sc[(size_t)(3 * r)] == in.sc[(size_t)(3 * r + 1)];
    const bool drop = loops && any;
    std::vector<std::vector<int64_t>> lists((size_t)slots);
    for (int64_t s = 0; s < S; ++s)
        for (int64_t r = in.ptr[(size_t)s]; r < in.ptr[(size_t)s + 1]; ++r) {
            const double vi = in.sc[(size_t)(3 * r)], vj = in.sc[(size_t)(3 * r + 1)];
            if (drop && vi == vj) continue;
            lists[(size_t)((s / G) * N + (int64_t)(transpose ? vi : vj))].push_back(r);
        }
    int64_t total = 0, nch = 0;
    for (int64_t s = 0; s < slots; ++s) {
        const std::vector<int64_t>& l = lists[(size_t)s];
        if (off[(size_t)s] != total || off[(size_t)s + 1] - off[(size_t)s] != (int64_t)l.size()) return 1;
        for (size_t e = 0; e < l.size(); ++e)
            if (rid[(size_t)total + e] != (int32_t)in.sc[(size_t)(3 * l[e] + (transpose ? 1 : 0))]) return 2;
        total += (int64_t)l.size();
        if ((int64_t)l.size() > spmm::CHUNK) {
            if (plan::dir_first(chunks, s, [&](int64_t q) { return dslot[(size_t)q]; }) != nch) return 3;
            nch += spmm::num_chunks((int64_t)l.size());
        }
    }
    if (ent != total || chunks != nch) return 4;
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    std::vector<Input> inputs = {hand(), star(515), batch()};
    Input empty{"empty", {}, {0, 0, 0}, {}, 5, 0};
    inputs.push_back(empty);
    Input range = hand();
    range.name = "id out of range"; range.sc[3 * 4] = 9.0; range.want = E_INDEX_RANGE;
    inputs.push_back(range);
    Input frac = hand();
    frac.name = "id 1.5"; frac.sc[3 * 2 + 1] = 1.5; frac.want = E_INDEX_RANGE;
    inputs.push_back(frac);
    Input past = hand();
    past.name = "ptr past m"; past.ptr = {0, 11, 11, 40}; past.want = E_BAD_ARG;
    inputs.push_back(past);
    Input cross = batch();
    cross.name = "id of another graph"; cross.sc[3 * 3] = 1.0; cross.want = E_INDEX_RANGE;
    inputs.push_back(cross);
    for (const Input& in : inputs)
        for (int flags = 0; flags < 8; ++flags)
            for (int transpose = 0; transpose < 2; ++transpose) {
                const int rc = check(in, flags, transpose);
                std::printf("%s flags %d transpose %d: %s (%d)%s\n", in.name, flags, transpose, rc ? "FAILED" : "ok", rc,
                            in.want ? " refused as expected" : "");
                bad |= rc;
            }
    return bad ? 1 : 0;
}
#endif
