// The host mirror of the sparse first layer (rlap_amd/csrc/rlap_featlin.h with rlap_plan.h and rlap_spmm.h): a whole feature plan
// buffer built on the host, and both products over it, every value from the header's functions.  Built by g++ -ffp-contract=off
// (tests/featlin_mirror.py) and, inside tests/csrc/featlin_main.cc, under the sanitizers.  The planned calls read the buffer as the
// kernels do: the parts must lie inside the bytes given, and every offset and id read from it is clamped.
#include <cstdint>
#include <cstring>
#include <vector>

#include "rlap_featlin.h"

using namespace rlap;

namespace {

// desc[]: what rlap_feature_desc holds
enum { D_N = 0, D_FIN, D_NNZ, D_CHUNKS_F, D_CHUNKS_T, D_OFF_F, D_DIR_F, D_REC_F, D_OFF_T, D_DIR_T, D_REC_T, D_BYTES, D_WORDS };

inline double x_at(const void* x, int f32, int64_t at) {
    return f32 ? (double)static_cast<const float*>(x)[at] : static_cast<const double*>(x)[at];
}

struct Part {
    const int64_t* off; const plan::Record* rec; const plan::ChunkRef* dir;
    int64_t slots, ids, entries, chunks;
};

// one direction of a buffer of `bytes` bytes, or false when its parts do not lie inside
bool part_of(const uint8_t* buf, int64_t bytes, const int64_t* d, int t, Part* p) {
    const int64_t have = d[D_BYTES] < bytes ? d[D_BYTES] : bytes;
    p->slots = t ? d[D_FIN] : d[D_N];
    p->ids = t ? d[D_N] : d[D_FIN];
    p->entries = d[D_NNZ];
    p->chunks = t ? d[D_CHUNKS_T] : d[D_CHUNKS_F];
    const int64_t off = t ? d[D_OFF_T] : d[D_OFF_F], dir = t ? d[D_DIR_T] : d[D_DIR_F], rec = t ? d[D_REC_T] : d[D_REC_F];
    if (p->ids < 1 || !featlin::parts_inside(p->slots, p->entries, p->chunks, off, dir, rec, d[D_NNZ], have)) return false;
    p->off = reinterpret_cast<const int64_t*>(buf + off);
    p->dir = reinterpret_cast<const plan::ChunkRef*>(buf + dir);
    p->rec = reinterpret_cast<const plan::Record*>(buf + rec);
    return true;
}

inline void list_of(const Part& p, int64_t slot, int64_t* o0, int64_t* n) {
    *o0 = featlin::clamp(p.off[slot], 0, p.entries);
    *n = featlin::clamp(p.off[slot + 1], *o0, p.entries) - *o0;
}

inline int64_t id_of(const Part& p, int64_t e) { return featlin::clamp(p.rec[e].id, 0, p.ids - 1); }

template <class T>
void forward(const Part& p, const T* w, const uint8_t* keep, int64_t K, int64_t F, T* y) {
    const int64_t N = p.slots, Fin = p.ids;
    for (int64_t k = 0; k < K; ++k)
        for (int64_t i = 0; i < N; ++i) {
            int64_t o0, n;
            list_of(p, i, &o0, &n);
            for (int64_t f = 0; f < F; ++f)
                y[(k * N + i) * F + f] = (T)featlin::forward_value(
                    n, [&](int64_t e) { return p.rec[o0 + e].c; }, [&](int64_t e) { return (double)w[id_of(p, o0 + e) * F + f]; },
                    [&](int64_t e) { return !keep || keep[k * Fin + id_of(p, o0 + e)] != 0; });
        }
}

template <class T>
void transposed(const Part& p, const T* g, const uint8_t* keep, int64_t K, int64_t F, T* dw) {
    const int64_t Fin = p.slots, N = p.ids;
    for (int64_t j = 0; j < Fin; ++j) {
        int64_t o0, n;
        list_of(p, j, &o0, &n);
        for (int64_t f = 0; f < F; ++f)
            dw[j * F + f] = (T)featlin::transposed_value(
                (int)K, [&](int k) { return !keep || keep[(int64_t)k * Fin + j] != 0; },
                [&](int k) {
                    return spmm::list_sum(
                        n, [&](int64_t e) { return p.rec[o0 + e].c; },
                        [&](int64_t e) { return (double)g[((int64_t)k * N + id_of(p, o0 + e)) * F + f]; }, false, 0.0, 0.0);
                });
    }
}

}  // namespace

extern "C" {

int featlin_chunk() { return spmm::CHUNK; }
int featlin_max_views() { return featlin::MAX_VIEWS; }
int featlin_magic() { return featlin::MAGIC; }

// out[7]: off forward / transposed, dir forward / transposed, rec forward / transposed, bytes
void featlin_layout(int64_t N, int64_t Fin, int64_t nnz, int forward_, int transposed_, int64_t* out) {
    const featlin::Layout L = featlin::layout(N, Fin, nnz, forward_ != 0, transposed_ != 0);
    out[0] = L.off[0]; out[1] = L.off[1]; out[2] = L.dir[0]; out[3] = L.dir[1]; out[4] = L.rec[0]; out[5] = L.rec[1]; out[6] = L.bytes;
}

int64_t featlin_count(const void* x, int f32, int64_t N, int64_t Fin) {
    int64_t c = 0;
    for (int64_t at = 0; at < N * Fin; ++at) c += featlin::kept(x_at(x, f32, at)) ? 1 : 0;
    return c;
}

// The whole build into buf (bytes >= the layout's).  desc[D_WORDS] as above; info[6]: longest forward / transposed, long lists
// forward / transposed (-1: not built), 0, 0.  Returns 0, or 3 when nnz is not the matrix's count or the buffer is too small.
int featlin_build(const void* x, int f32, int64_t N, int64_t Fin, int64_t nnz, int forward_, int transposed_, uint8_t* buf, int64_t bytes,
                  int64_t* desc, int64_t* info) {
    for (int k = 0; k < D_WORDS; ++k) desc[k] = 0;
    if (N < 1 || Fin < 1 || nnz < 0 || featlin_count(x, f32, N, Fin) != nnz) return 3;
    const bool want[2] = {forward_ != 0, transposed_ != 0};
    const featlin::Layout L = featlin::layout(N, Fin, nnz, want[0], want[1]);
    if (L.bytes > bytes) return 3;
    const int64_t slots[2] = {N, Fin}, dcap = plan::dir_cap(nnz);
    int64_t chunks[2] = {-1, -1};
    for (int d = 0; d < 2; ++d) {
        info[d] = info[2 + d] = -1;
        if (!want[d]) continue;
        int64_t* off = reinterpret_cast<int64_t*>(buf + L.off[d]);
        plan::Record* rec = reinterpret_cast<plan::Record*>(buf + L.rec[d]);
        plan::ChunkRef* dir = reinterpret_cast<plan::ChunkRef*>(buf + L.dir[d]);
        int64_t at = 0, first = 0, longest = 0, long_lists = 0;
        for (int64_t s = 0; s < slots[d]; ++s) {
            off[s] = at;
            const int64_t others = d ? N : Fin;
            for (int64_t o = 0; o < others; ++o) {   // ascending column (forward) or row (transposed)
                const double v = d ? x_at(x, f32, o * Fin + s) : x_at(x, f32, s * Fin + o);
                if (!featlin::kept(v)) continue;
                plan::Record r;
                std::memset(&r, 0, sizeof(r));
                r.c = v; r.id = (int32_t)o; r.zero = 0;
                rec[at++] = r;
            }
            const int64_t len = at - off[s];
            longest = len > longest ? len : longest;
            long_lists += plan::dir_chunks(len) > 0 ? 1 : 0;
            plan::dir_write(s, len, first, dcap, [&](int64_t q, plan::ChunkRef c) { dir[q] = c; });
            first += plan::dir_chunks(len);
        }
        off[slots[d]] = at;
        chunks[d] = first;
        info[d] = longest;
        info[2 + d] = long_lists;
    }
    info[4] = info[5] = 0;
    desc[D_N] = N; desc[D_FIN] = Fin; desc[D_NNZ] = nnz; desc[D_CHUNKS_F] = chunks[0]; desc[D_CHUNKS_T] = chunks[1];
    desc[D_OFF_F] = L.off[0]; desc[D_DIR_F] = L.dir[0]; desc[D_REC_F] = L.rec[0];
    desc[D_OFF_T] = L.off[1]; desc[D_DIR_T] = L.dir[1]; desc[D_REC_T] = L.rec[1];
    desc[D_BYTES] = L.bytes;
    return 0;
}

// A planned call on a buffer of `bytes` bytes.  Forward: w (Fin, F), out (K, N, F); transposed: w is G (K, N, F), out (Fin, F).
// keep (K, Fin) or null (K = 1).  Returns 0, or 3 for a bad K, a direction the buffer lacks or parts outside the buffer.
int featlin_apply(const uint8_t* buf, int64_t bytes, const int64_t* desc, int transpose, int f32, const void* w, const uint8_t* keep, int64_t K,
                  int64_t F, void* out) {
    if (K < 1 || K > featlin::MAX_VIEWS || (!keep && K != 1) || F < 1) return 3;
    Part p;
    if (!part_of(buf, bytes, desc, transpose ? 1 : 0, &p)) return 3;
    if (transpose) {
        if (f32) transposed<float>(p, static_cast<const float*>(w), keep, K, F, static_cast<float*>(out));
        else transposed<double>(p, static_cast<const double*>(w), keep, K, F, static_cast<double*>(out));
    } else {
        if (f32) forward<float>(p, static_cast<const float*>(w), keep, K, F, static_cast<float*>(out));
        else forward<double>(p, static_cast<const double*>(w), keep, K, F, static_cast<double*>(out));
    }
    return 0;
}

// the first directory number of `slot` (plan::dir_first over the direction's directory), or -1 when the parts lie outside
int64_t featlin_dir_first(const uint8_t* buf, int64_t bytes, const int64_t* desc, int transpose, int64_t slot) {
    Part p;
    if (!part_of(buf, bytes, desc, transpose ? 1 : 0, &p)) return -1;
    return plan::dir_first(p.chunks, slot, [&](int64_t q) { return p.dir[q].slot; });
}

}  // extern "C"
