// Host mirror of a propagation plan's layout rules: rlap_amd/csrc/rlap_plan.h -- the very header rlap_plan.hip includes -- compiled
// with g++ -ffp-contract=off.  plan_build lays the lists of one direction out as the device build does (the same slot, place,
// record-index and directory functions), from rows and one coefficient per row; plan_product sums them by rlap_spmm.h's rule.
// tests/test_plan_cpu.py checks both against a straightforward Python construction and against tests/csrc/spmm_mirror.cc.
// With -DPLAN_MIRROR_MAIN the file is a stand-alone program that builds the plans of a hand-made input and of a star with 600
// leaves and checks them against lists built the plain way: it is what runs under -fsanitize=address,undefined.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "rlap_plan.h"

using namespace rlap;

extern "C" {

int64_t plan_record_bytes() { return (int64_t)sizeof(plan::Record); }
int64_t plan_chunkref_bytes() { return (int64_t)sizeof(plan::ChunkRef); }
int64_t plan_dir_cap(int64_t m) { return plan::dir_cap(m); }

// loop, off[2], dir[2], rec[2], bytes
void plan_layout(int64_t m, int64_t slots, int loops, int forward, int transposed, int64_t* out) {
    const plan::Layout L = plan::layout(m, slots, loops != 0, forward != 0, transposed != 0);
    out[0] = L.loop; out[1] = L.off[0]; out[2] = L.off[1]; out[3] = L.dir[0]; out[4] = L.dir[1]; out[5] = L.rec[0]; out[6] = L.rec[1];
    out[7] = L.bytes;
}

// The lists of one direction.  sc (m, 3) rows [row, col, w] grouped by column within the S segments of ptr, L = S / G layers of N
// ids, c[r] the coefficient of row r; drop: loop rows leave the lists.  Writes off[L N + 1], the records (rec_c, rec_id, m each at
// most) and the directory (dir_slot, dir_k, dir_cap(m) each at most); returns the records, *chunks the directory entries.
int64_t plan_build(int64_t m, const double* sc, int64_t S, const int64_t* ptr, int64_t G, int64_t N, const double* c, int drop,
                   int transpose, int64_t* off, double* rec_c, int32_t* rec_id, int64_t* dir_slot, int64_t* dir_k, int64_t* chunks) {
    const int64_t slots = (S / G) * N;
    std::vector<int64_t> layer((size_t)m), order((size_t)m), slot((size_t)m);
    for (int64_t s = 0; s < S; ++s)
        for (int64_t r = ptr[s]; r < ptr[s + 1]; ++r) layer[(size_t)r] = s / G;
    // the list an entry is in: its target's (forward) or its source's (transposed)
    for (int64_t r = 0; r < m; ++r) slot[(size_t)r] = plan::slot_of(layer[(size_t)r], N, (int64_t)sc[3 * r + (transpose ? 0 : 1)]);
    // positions: the rows as they are (forward: a list is a column block), or stably sorted by the list they are in (transposed)
    std::iota(order.begin(), order.end(), (int64_t)0);
    if (transpose) std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return slot[(size_t)a] < slot[(size_t)b]; });
    auto is_loop = [&](int64_t p) { const int64_t r = order[(size_t)p]; return sc[3 * r] == sc[3 * r + 1]; };
    std::vector<int64_t> first((size_t)m);   // the first position of the list of position p
    for (int64_t p = 0; p < m; ++p)
        first[(size_t)p] = (p > 0 && slot[(size_t)order[(size_t)p - 1]] == slot[(size_t)order[(size_t)p]]) ? first[(size_t)p - 1] : p;
    std::vector<int64_t> kept((size_t)slots + 1, 0);
    for (int64_t p = 0; p < m; ++p) kept[(size_t)slot[(size_t)order[(size_t)p]]] += (drop && is_loop(p)) ? 0 : 1;
    off[0] = 0;
    for (int64_t s = 0; s < slots; ++s) off[s + 1] = off[s] + kept[(size_t)s];
    for (int64_t p = 0; p < m; ++p) {
        if (drop && is_loop(p)) continue;
        const int64_t r = order[(size_t)p], s = slot[(size_t)r], f = first[(size_t)p];
        const int64_t place = drop ? plan::place_counting(p - f, [&](int64_t j) { return is_loop(f + j); }) : plan::place_plain(f, p);
        const int64_t at = plan::record_index(off[s], off[s + 1], place);
        if (at < 0) return -1;
        rec_c[at] = c[r];
        rec_id[at] = (int32_t)sc[3 * r + (transpose ? 1 : 0)];
    }
    int64_t q = 0;
    for (int64_t s = 0; s < slots; ++s) {
        plan::dir_write(s, kept[(size_t)s], q, plan::dir_cap(m), [&](int64_t at, plan::ChunkRef ref) { dir_slot[at] = ref.slot; dir_k[at] = ref.k; });
        q += plan::dir_chunks(kept[(size_t)s]);
    }
    *chunks = q;
    return off[slots];
}

// the first directory number of a slot's list
int64_t plan_dir_first(int64_t chunks, const int64_t* dir_slot, int64_t slot) {
    return plan::dir_first(chunks, slot, [&](int64_t q) { return dir_slot[q]; });
}

// y (slots, F) from the lists of one direction: x (N, F) shared by the layers, loopc[slots] the loop coefficients (loops != 0).
// A long list is summed through the directory: chunk by chunk, by the numbers its slot has there.
int plan_product(int64_t slots, int64_t N, int64_t F, const int64_t* off, const double* rec_c, const int32_t* rec_id, int64_t chunks,
                 const int64_t* dir_slot, const int64_t* dir_k, const double* x, int loops, const double* loopc, double* y) {
    for (int64_t s = 0; s < slots; ++s) {
        const int64_t o0 = off[s], n = off[s + 1] - off[s], id = s % N;
        for (int64_t f = 0; f < F; ++f) {
            auto coef = [&](int64_t e) { return rec_c[o0 + e]; };
            auto feat = [&](int64_t e) { return x[(int64_t)rec_id[o0 + e] * F + f]; };
            double total = spmm::list_sum(n, coef, feat, loops != 0, loops ? loopc[s] : 0.0, x[id * F + f]);
            if (plan::dir_chunks(n) > 0) {   // the same sum as the chunk kernel and the rows kernel split it
                const int64_t q0 = plan_dir_first(chunks, dir_slot, s);
                double t = 0.0;
                for (int64_t k = 0; k < spmm::num_chunks(n); ++k) {
                    if (q0 + k >= chunks || dir_slot[q0 + k] != s || dir_k[q0 + k] != k) return 1;
                    t = t + spmm::chunk_sum(n, dir_k[q0 + k], coef, feat);
                }
                if (loops) t = spmm::accumulate(t, loopc[s], x[id * F + f]);
                if (t != total) return 2;
            }
            y[s * F + f] = total;
        }
    }
    return 0;
}

}  // extern "C"

#ifdef PLAN_MIRROR_MAIN
#include <cstdio>

namespace {

struct Input { std::vector<double> sc; std::vector<int64_t> ptr; int64_t N; };

Input hand() {   // two loop rows of id 0, an id with nothing but a loop row; twice, as two layers
    const double rows[8][3] = {{1, 0, 0.5}, {0, 0, 3.0}, {2, 0, 0.25}, {0, 0, 4.0}, {0, 1, 0.5}, {0, 2, 0.25}, {2, 2, 7.0}, {5, 5, 2.0}};
    Input in;
    for (int rep = 0; rep < 2; ++rep)
        for (auto& r : rows) in.sc.insert(in.sc.end(), r, r + 3);
    in.ptr = {0, 8, 16};
    in.N = 7;
    return in;
}

Input star(int64_t leaves) {   // the centre's block with two loop rows inside, then one block per leaf
    Input in;
    for (int64_t i = 0; i < leaves; ++i) {
        if (i == 3 || i == 300) { const double l[3] = {0, 0, 1.5}; in.sc.insert(in.sc.end(), l, l + 3); }
        const double r[3] = {(double)(i + 1), 0, 0.5 + 0.001 * (double)i};
        in.sc.insert(in.sc.end(), r, r + 3);
    }
    for (int64_t i = 0; i < leaves; ++i) { const double r[3] = {0, (double)(i + 1), 0.5 + 0.001 * (double)i}; in.sc.insert(in.sc.end(), r, r + 3); }
    in.ptr = {0, (int64_t)in.sc.size() / 3};
    in.N = leaves + 1;
    return in;
}

int check(const Input& in, int drop, int transpose) {
    const int64_t m = (int64_t)in.sc.size() / 3, S = (int64_t)in.ptr.size() - 1, N = in.N, slots = S * N;
    std::vector<double> c((size_t)m);
    for (int64_t r = 0; r < m; ++r) c[(size_t)r] = 0.25 + 0.5 * (double)(r % 7);
    std::vector<int64_t> off((size_t)slots + 1), dslot((size_t)plan::dir_cap(m)), dk((size_t)plan::dir_cap(m));
    std::vector<double> rc((size_t)m);
    std::vector<int32_t> rid((size_t)m);
    int64_t chunks = -1;
    const int64_t ent = plan_build(m, in.sc.data(), S, in.ptr.data(), 1, N, c.data(), drop, transpose, off.data(), rc.data(), rid.data(),
                                   dslot.data(), dk.data(), &chunks);
    // the plain way: every list by appending in input order
    std::vector<std::vector<int64_t>> lists((size_t)slots);
    for (int64_t s = 0; s < S; ++s)
        for (int64_t r = in.ptr[(size_t)s]; r < in.ptr[(size_t)s + 1]; ++r) {
            const double vi = in.sc[(size_t)(3 * r)], vj = in.sc[(size_t)(3 * r + 1)];
            if (drop && vi == vj) continue;
            lists[(size_t)(s * N + (int64_t)(transpose ? vi : vj))].push_back(r);
        }
    int64_t total = 0, nch = 0;
    for (int64_t s = 0; s < slots; ++s) {
        const std::vector<int64_t>& l = lists[(size_t)s];
        if (off[(size_t)s] != total || off[(size_t)s + 1] - off[(size_t)s] != (int64_t)l.size()) return 1;
        for (size_t e = 0; e < l.size(); ++e) {
            const int64_t r = l[e];
            if (rc[(size_t)total + e] != c[(size_t)r] || rid[(size_t)total + e] != (int32_t)in.sc[(size_t)(3 * r + (transpose ? 1 : 0))]) return 2;
        }
        total += (int64_t)l.size();
        if ((int64_t)l.size() > spmm::CHUNK) {
            if (plan_dir_first(chunks, dslot.data(), s) != nch) return 3;
            nch += spmm::num_chunks((int64_t)l.size());
        }
    }
    if (ent != total || chunks != nch) return 4;
    std::vector<double> x((size_t)(N * 2)), loopc((size_t)slots, 0.75), y((size_t)(slots * 2));
    for (size_t i = 0; i < x.size(); ++i) x[i] = 1.0 / (double)(i + 3);
    if (plan_product(slots, N, 2, off.data(), rc.data(), rid.data(), chunks, dslot.data(), dk.data(), x.data(), drop, loopc.data(), y.data())) return 5;
    return 0;
}

}  // namespace

int main() {
    int bad = 0;
    const Input inputs[2] = {hand(), star(600)};
    for (int i = 0; i < 2; ++i)
        for (int drop = 0; drop < 2; ++drop)
            for (int transpose = 0; transpose < 2; ++transpose) {
                const int rc = check(inputs[i], drop, transpose);
                std::printf("input %d drop %d transpose %d: %s (%d)\n", i, drop, transpose, rc ? "FAILED" : "ok", rc);
                bad |= rc;
            }
    return bad ? 1 : 0;
}
#endif
