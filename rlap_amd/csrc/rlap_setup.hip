// rlap_setup.hip -- the setup kernels of a call, in front of the round kernels (rlap_kernels.hip).
//
//   K10 k_mt19937_64_table   sampling stream of preconditioner.cc:356-357
//   K1  k_edge_keys/k_heads/k_fill_csr   COO -> CSR  (reader.cc:42-61)
//   K2+K3 k_twin_sorted      symmetry check + twin index (factorizers.cc:19-22,
//                            preconditioner.cc:22-49)
//   K4  k_pq_init/k_bucket_bounds  bucket queue (preconditioner.cc:125-165)
//   k_views_replicate        K views of the input in one arena
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rlap_core.h"
#include "rlap_kernels.h"

namespace rlap {

// ---------------------------------------------------------------------------
// K10: MT19937-64 (default seed 5489) -> u = (double)raw / 2^64, clamped below 1
// (libstdc++ generate_canonical, bits/random.tcc:3348-3380).  One workgroup.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(320) void k_mt19937_64_table(double* __restrict__ out, int64_t count) {
    constexpr int NN = 312, MM = 156;
    constexpr uint64_t MATRIX_A = 0xB5026F5AA96619E9ull, UM = 0xFFFFFFFF80000000ull, LM = 0x7FFFFFFFull;
    __shared__ uint64_t x[NN];
    const int tid = threadIdx.x;
    if (tid == 0) {
        uint64_t s = 5489ull;
        x[0] = s;
        for (int i = 1; i < NN; ++i) { s = 6364136223846793005ull * (s ^ (s >> 62)) + (uint64_t)i; x[i] = s; }
    }
    __syncthreads();
    for (int64_t base = 0; base < count; base += NN) {
        // twist, first half: inputs are all old words
        uint64_t nv = 0;
        if (tid < MM) {
            uint64_t y = (x[tid] & UM) | (x[tid + 1] & LM);
            nv = x[tid + MM] ^ (y >> 1) ^ ((y & 1ull) ? MATRIX_A : 0ull);
        }
        __syncthreads();
        if (tid < MM) x[tid] = nv;
        __syncthreads();
        // second half: x[i-156] is new, x[i+1] old (x[0] new for i = 311)
        if (tid >= MM && tid < NN) {
            uint64_t nxt = x[(tid + 1) % NN];
            uint64_t y = (x[tid] & UM) | (nxt & LM);
            nv = x[tid - MM] ^ (y >> 1) ^ ((y & 1ull) ? MATRIX_A : 0ull);
        }
        __syncthreads();
        if (tid >= MM && tid < NN) x[tid] = nv;
        __syncthreads();
        if (tid < NN && base + tid < count) {
            uint64_t y = x[tid];
            y ^= (y >> 29) & 0x5555555555555555ull;
            y ^= (y << 17) & 0x71D67FFFEDA60000ull;
            y ^= (y << 37) & 0xFFF7EEE000000000ull;
            y ^= (y >> 43);
            double u = (double)y * 5.42101086242752217003726400434970855712890625e-20;  // 2^-64
            if (u >= 1.0) u = 0.99999999999999988897769753748434595763683319091796875;
            out[base + tid] = u;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// identity / edge_info helpers (py_api_binder.cc:10-51,71-76; ops.py:47)
// ---------------------------------------------------------------------------
__global__ void k_transpose_copy(const double* __restrict__ in, double* __restrict__ out, int64_t rows, int64_t cols, int to_colmajor) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = rows * cols;
    if (i >= total) return;
    int64_t r = i / cols, c = i % cols;
    if (to_colmajor) out[c * rows + r] = in[i]; else out[i] = in[c * rows + r];
}

__global__ void k_unpack_edge_info(const double* __restrict__ ei, int64_t E, int64_t* __restrict__ row, int64_t* __restrict__ col, double* __restrict__ w) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= E) return;
    row[p] = (int64_t)ei[3 * p];
    col[p] = (int64_t)ei[3 * p + 1];
    w[p] = ei[3 * p + 2];
}

// Exchange format of sc_edge_info between GPUs (the RCCL all-gather): a row [row, col, w] as two 64-bit
// words -- (row << 32 | col), the bits of w -- 16 bytes over xGMI instead of 24.  One thread per row, both directions.
__global__ void k_pack_rows(const double* __restrict__ sc, int64_t m, unsigned long long* __restrict__ packed) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const unsigned long long r = (unsigned long long)(long long)sc[3 * p], c = (unsigned long long)(long long)sc[3 * p + 1];
    packed[2 * p] = (r << 32) | (c & 0xFFFFFFFFull);
    packed[2 * p + 1] = (unsigned long long)__double_as_longlong(sc[3 * p + 2]);
}
__global__ void k_unpack_rows(const unsigned long long* __restrict__ packed, int64_t m, double* __restrict__ sc) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const unsigned long long ids = packed[2 * p];
    sc[3 * p] = (double)(ids >> 32);
    sc[3 * p + 1] = (double)(ids & 0xFFFFFFFFull);
    sc[3 * p + 2] = __longlong_as_double((long long)packed[2 * p + 1]);
}

// ---------------------------------------------------------------------------
// K1: COO -> CSR
// ---------------------------------------------------------------------------
__global__ void k_vertex_graph(const int64_t* __restrict__ node_ptr, int G, int32_t* __restrict__ vgraph, int64_t N) {
    int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= N) return;
    int lo = 0, hi = G;  // last g with node_ptr[g] <= v
    while (hi - lo > 1) {
        int mid = (lo + hi) >> 1;
        if (node_ptr[mid] <= v) lo = mid; else hi = mid;
    }
    vgraph[v] = lo;
}

// symmetrize != 0: the step before the path (PyG to_undirected, scripts/node_shared.py:326-327) fused in -- every
// input entry (a,b) also yields (b,a); the duplicates this creates are folded by k_heads / k_fill_csr.
__global__ void k_edge_keys(const int64_t* __restrict__ row, const int64_t* __restrict__ col, const double* __restrict__ w,
                            int64_t E, int64_t N, const int32_t* __restrict__ vgraph, int symmetrize, int kbits, uint64_t* __restrict__ keys,
                            uint32_t* __restrict__ idx, int32_t* __restrict__ flags) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t Eeff = symmetrize ? 2 * E : E;
    if (p >= Eeff) return;
    const int64_t q = p < E ? p : p - E;
    int64_t r = row[q], c = col[q];
    if (p >= E) { const int64_t t = r; r = c; c = t; }
    double wv = w ? w[q] : 1.0;
    uint64_t k = ~0ull;
    if (r < 0 || r >= N || c < 0 || c >= N) {
        flags[FLAG_RANGE] = 1;
    } else if (wv != 0) {
        if (vgraph && vgraph[r] != vgraph[c]) flags[FLAG_CROSS] = 1;
        k = ((uint64_t)c << kbits) | (uint64_t)r;   // kbits = bits of N - 1: the sort only runs over the 2 * kbits + 1 bits that can differ
    }
    keys[p] = k;
    idx[p] = (uint32_t)q;
    // is the input in (col, row) order already -- or in (row, col) order, what PyG's coalesce leaves?  (Then the radix sort
    // can be skipped, rlap_api.hip.)  Every entry is compared with its predecessor in both orders.
    if (!symmetrize && p > 0) {
        const int64_t r0 = row[p - 1], c0 = col[p - 1];
        const double w0 = w ? w[p - 1] : 1.0;
        const bool bad = (k == ~0ull) || w0 == 0 || r0 < 0 || r0 >= N || c0 < 0 || c0 >= N;
        if (bad || (((uint64_t)c0 << kbits) | (uint64_t)r0) > k) flags[FLAG_UNSORTED_CR] = 1;
        if (bad || (((uint64_t)r0 << kbits) | (uint64_t)c0) > (((uint64_t)r << kbits) | (uint64_t)c)) flags[FLAG_UNSORTED_RC] = 1;
    } else if (p == 0 && k == ~0ull) { flags[FLAG_UNSORTED_CR] = 1; flags[FLAG_UNSORTED_RC] = 1; }
}

// num_nodes = edge_index.max() + 1 (scripts/augmentor_benchmarks.py:77) without a torch reduction + .item()
__global__ void k_max_id(const int64_t* __restrict__ row, const int64_t* __restrict__ col, int64_t E, unsigned long long* __restrict__ out) {
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    long long m = -1;
    bool neg = false;
    for (; p < E; p += (int64_t)gridDim.x * blockDim.x) { long long r = row[p], c = col[p]; m = r > m ? r : m; m = c > m ? c : m; neg |= (r < 0) | (c < 0); }
    for (int off = 32; off > 0; off >>= 1) { long long o = __shfl_down(m, off); m = o > m ? o : m; }
    if ((threadIdx.x & 63) == 0 && m >= 0) atomicMax(out, (unsigned long long)(m + 1));
    if (neg) out[1] = 1ull;   // a negative id: out of range whatever num_nodes is
}

// several small fills in one launch (per-call state that used to take a dozen memsets)
__global__ void k_fill_multi(FillJobs J) {
    const int j = blockIdx.y;
    if (j >= J.n) return;
    int32_t* p = J.ptr[j];
    const int64_t cnt = J.count[j];
    const int32_t v = J.value[j];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) p[i] = v;
}

// o_v = random: the injected node_id vector must hold, per graph, a permutation of its LOCAL ids
// (preconditioner.cc:588-601 builds 0..n-1 and shuffles it); anything else would index out of bounds.
__global__ void k_perm_check(const int64_t* __restrict__ perm, const int32_t* __restrict__ vgraph, const GraphDesc* __restrict__ gd,
                             int32_t N, int32_t* __restrict__ seen, int32_t* __restrict__ flags) {
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const GraphDesc& D = gd[vgraph[i]];
    const int64_t p = perm[i];
    if (p < 0 || p >= (int64_t)D.n) { flags[FLAG_PERM] = 1; return; }
    if (atomicExch(&seen[D.vbase + (int32_t)p], 1) != 0) flags[FLAG_PERM] = 1;
}

// per-graph scratch for the long-column fall-backs: nnz_g / 2 + 8 entries each, bases by a running sum
// (one workgroup; the per-graph nnz is only known on the device)
__global__ __launch_bounds__(256) void k_gd_scratch(const int32_t* __restrict__ colptr, const int64_t* __restrict__ node_ptr, int32_t G,
                                                    GraphDesc* __restrict__ gd) {
    __shared__ int32_t s_w[4];
    __shared__ int32_t s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (int32_t g0 = 0; g0 < G; g0 += 256) {
        const int32_t g = g0 + tid;
        int32_t sc = 0;
        if (g < G) sc = (colptr[node_ptr[g + 1]] - colptr[node_ptr[g]]) / 2 + 8;
        int32_t incl = sc;
        for (int off = 1; off < 64; off <<= 1) { int32_t t = __shfl_up(incl, off); if (lane >= off) incl += t; }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        int32_t base = s_carry;
        for (int w = 0; w < wv; ++w) base += s_w[w];
        if (g < G) { gd[g].scr_base = base + incl - sc; gd[g].scr_cap = sc; }
        __syncthreads();
        if (tid == 255) s_carry = base + incl;
        __syncthreads();
    }
}

// everything the host wants to know about a call, gathered into one block (one D2H copy at the end)
__global__ __launch_bounds__(256) void k_collect(const int32_t* __restrict__ flags, const double* __restrict__ acc, const int32_t* __restrict__ nnz_p,
                          const unsigned long long* __restrict__ counters, const unsigned long long* __restrict__ live,
                          const int64_t* __restrict__ tmp_off, const int64_t* __restrict__ row_off,
                          int32_t S, const GraphDesc* __restrict__ gd, int32_t G, const int32_t* __restrict__ pool_top,
                          const int32_t* __restrict__ bs_pool_top, const int32_t* __restrict__ flow_reason,
                          const int32_t* __restrict__ sq_marks, int32_t n_sq, CallResults* __restrict__ out) {
    __shared__ int32_t s_st;
    __shared__ unsigned long long s_nd, s_rounds, s_singles;
    __shared__ int32_t s_narrow, s_nsq;
    const int tid = threadIdx.x;
    if (tid == 0) { s_st = 0; s_nd = 0ull; s_rounds = 0ull; s_singles = 0ull; s_narrow = 0; s_nsq = 0; }
    __syncthreads();
    int32_t st = 0, narrow = 0, nsq = 0; unsigned long long nd = 0, rounds = 0, singles = 0;
    for (int32_t g = tid; g < G; g += blockDim.x) {
        const int32_t sg = gd[g].status;
        if (sg > st) st = sg;
        const unsigned long long d = (unsigned long long)gd[g].n_draws;
        nd = d > nd ? d : nd;
        rounds += (unsigned long long)gd[g].pad0; singles += (unsigned long long)gd[g].pad1;
        narrow += gd[g].narrow_rounds;
        // squeeze pass p counts when the 16-slot kernel ran a round between it and the next pass (or the end): sq_marks[p * G + g] is
        // the graph's narrow_rounds when pass p ran
        for (int32_t p = 0; p < n_sq; ++p)
            if ((p + 1 < n_sq ? sq_marks[(p + 1) * G + g] : gd[g].narrow_rounds) > sq_marks[p * G + g]) ++nsq;
    }
    if (narrow) atomicAdd(&s_narrow, narrow);
    if (nsq) atomicAdd(&s_nsq, nsq);
    if (st) atomicMax(&s_st, st);
    if (nd) atomicMax(&s_nd, nd);
    if (rounds) atomicAdd(&s_rounds, rounds);
    if (singles) atomicAdd(&s_singles, singles);
    __syncthreads();
    if (tid != 0) return;
    CallResults R;
    for (int q = 0; q < FLAG_COUNT; ++q) R.flags[q] = flags[q];
    for (int q = 0; q < 4; ++q) R.acc[q] = acc[q];
    R.nnz = *nnz_p;
    { unsigned long long lt = 0ull; for (int q = 0; q < LIVE_SLOTS; ++q) lt += live[q * LIVE_STRIDE]; R.live_total = (int64_t)lt; }
    R.scr_need = (int64_t)counters[0];
    R.ext_total = tmp_off[S];
    R.m_total = row_off[S];
    R.pool_used = *pool_top;
    R.log_used = *bs_pool_top;
    R.status = s_st; R.n_draws = (int64_t)s_nd; R.rounds = (int64_t)s_rounds; R.singles = (int64_t)s_singles;
    R.flow_abort = flow_reason ? *flow_reason : 0; R.rounds_narrow = s_narrow;
    R.n_squeezes = s_nsq; R.pad = 0;
    *out = R;
}

__global__ void k_heads(const uint64_t* __restrict__ keys, int64_t E, int32_t* __restrict__ head) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > E) return;
    if (i == E) { head[E] = 0; return; }
    uint64_t k = keys[i];
    head[i] = (k != ~0ull && (i == 0 || keys[i - 1] != k)) ? 1 : 0;
}

__global__ void k_fill_csr(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ idx, const int32_t* __restrict__ head,
                           const int32_t* __restrict__ pos, const double* __restrict__ w, int64_t E, int set_semantics, int kbits,
                           Slot* __restrict__ ent, int32_t* __restrict__ slot_col, int32_t* __restrict__ nbr32) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E || !head[i]) return;
    uint64_t k = keys[i];
    int32_t s = pos[i];
    double sum = w ? w[idx[i]] : 1.0;
    // duplicates summed in input order (setFromTriplets); unweighted symmetrised input is an edge SET (PyG coalesce): weight 1
    if (!set_semantics) for (int64_t q = i + 1; q < E && keys[q] == k; ++q) sum += w ? w[idx[q]] : 1.0;
    int32_t c = (int32_t)(k >> kbits);
    Slot g; g.val = sum; g.nbr = (int32_t)(k & ((1ull << kbits) - 1ull)); g.twin = c;   // (twin holds the COLUMN until k_twin_store: k_twin_sorted reads a partner's ids and weight with one 16-byte load)
    ent[s] = g;
    slot_col[s] = c;
    nbr32[s] = g.nbr;   // dense copy of the row ids: key of the sort that finds the twins (k_twin_sorted)
}

// colptr[c] = first slot whose column is >= c (slots are sorted by column): no atomics, empty columns included
// (thread 0 also files the entry count where the later kernels read it and starts the append pool behind the CSR image:
//  two 4-byte device-to-device copies less per call)
__global__ void k_colptr(const int32_t* __restrict__ slot_col, const int32_t* __restrict__ nnz_p, int32_t N, int32_t* __restrict__ colptr,
                         int32_t* __restrict__ nnz_out, int32_t* __restrict__ pool_top_out) {
    int32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > N) return;
    if (c == 0) { const int32_t z = *nnz_p; *nnz_out = z; *pool_top_out = z; }
    int32_t lo = 0, hi = *nnz_p;
    while (lo < hi) {
        int32_t mid = (lo + hi) >> 1;
        if (slot_col[mid] < c) lo = mid + 1; else hi = mid;
    }
    colptr[c] = lo;
}

// ---------------------------------------------------------------------------
// K2 + K3: twin index (from one stable sort of the slots by row id) and
// the isApprox(A^T) test: ||A-A^T||_F^2 <= 1e-24 ||A||_F^2 (Eigen default prec).
// ---------------------------------------------------------------------------
// Twins from a sort instead of a search per entry.  The slots are in (col, row) order; a STABLE sort of the slots by
// row alone puts them in (row, col) order: T[k] = slot holding the k-th smallest (row, col) pair.  For a symmetric
// pattern that pair is the transpose of the k-th smallest (col, row) pair, i.e. of slot k: twin[k] = T[k].  Any slot whose
// partner does not hold the transposed ids proves the pattern asymmetric.  (One radix sort of 4-byte keys over bits_for(N)
// bits and two gathers per entry instead of log2(degree) dependent probes.)
__global__ __launch_bounds__(256) void k_twin_sorted(const Slot* __restrict__ ent, const uint32_t* __restrict__ T, const int32_t* __restrict__ nnz_p,
                                                     double* __restrict__ acc) {
    const int32_t nnz = *nnz_p;
    double d2 = 0, n2 = 0;
    bool asym = false;
    for (int32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += gridDim.x * blockDim.x) {
        const Slot me = ent[p];                  // (val, row, column)
        n2 += me.val * me.val;
        const uint32_t q = T[p];
        bool ok = q < (uint32_t)nnz;
        if (ok) {
            const Slot tw = ent[q];              // one 16-byte gather: the partner's weight, row and column
            ok = tw.nbr == me.twin && tw.twin == me.nbr;
            if (ok) { const double d = me.val - tw.val; d2 += d * d; }
        }
        if (!ok) { d2 += 2 * me.val * me.val; asym = true; }
    }
    if (asym) acc[2] = 1.0;  // structurally asymmetric
    for (int off = 32; off > 0; off >>= 1) { d2 += __shfl_down(d2, off); n2 += __shfl_down(n2, off); }
    __shared__ double sd[4], sn[4];
    int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sd[w] = d2; sn[w] = n2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double bd = sd[0] + sd[1] + sd[2] + sd[3], bn = sn[0] + sn[1] + sn[2] + sn[3];
        if (bd != 0.0) atomicAdd(&acc[0], bd);
        if (bn != 0.0) atomicAdd(&acc[1], bn);
    }
}
// ... and the twin indices stored once every partner has been read (the field held the column until now)
__global__ void k_twin_store(Slot* __restrict__ ent, const uint32_t* __restrict__ T, const int32_t* __restrict__ nnz_p) {
    const int32_t nnz = *nnz_p;
    for (int32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += gridDim.x * blockDim.x) ent[p].twin = (int32_t)T[p];
}

// Views (rlap_approx_chol_views): the CSR of the K-fold disjoint union of the input is the input's CSR shifted by view --
// columns are sorted by global id and rows within a column too, so copy k's slots come after copy k-1's, in the same order,
// with the same twin links.  The setup ran on copy 0; this writes copies 1..K-1 of every slot (16-byte records), slot column
// and column start, and sets the entry count and the append pool's first free slot to K * nnz.  A streaming copy: each source
// element is read once and stored K-1 times, grid-stride, no LDS.  Reads [0, nnz) / [0, N) and writes [nnz, K nnz) / [N, K N].
__global__ __launch_bounds__(256) void k_views_replicate(Slot* ent, int32_t* slot_col, int32_t* colptr, const int32_t* __restrict__ nnz_src,
                                                         int32_t N, int32_t K, int32_t* __restrict__ nnz_out, int32_t* __restrict__ pool_top_out) {
    const int32_t nnz = *nnz_src;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (tid == 0) { const int32_t z = K * nnz; *nnz_out = z; *pool_top_out = z; colptr[(int64_t)K * N] = z; }
    uint4* e4 = reinterpret_cast<uint4*>(ent);   // Slot = {double val; int32 nbr; int32 twin}: words x,y = val, z = nbr, w = twin
    for (int64_t p = tid; p < nnz; p += stride) {
        uint4 v = e4[p];
        const uint32_t nbr = v.z, twin = v.w;
        const int32_t c = slot_col[p];
        for (int32_t k = 1; k < K; ++k) {
            v.z = nbr + (uint32_t)(k * N); v.w = twin + (uint32_t)(k * nnz);
            e4[(int64_t)k * nnz + p] = v;
            slot_col[(int64_t)k * nnz + p] = c + k * N;
        }
    }
    for (int64_t v = tid; v < N; v += stride) {
        const int32_t c0 = colptr[v];
        for (int32_t k = 1; k < K; ++k) colptr[(int64_t)k * N + v] = c0 + k * nnz;
    }
}

// ---------------------------------------------------------------------------
// K4: PQ init.  Keys = degree; never-moved vertices of a bucket are listed in
// descending id (= LIFO order after ascending insertion, :137-157).
// ---------------------------------------------------------------------------
__global__ void k_pq_init(const int32_t* __restrict__ colptr, const int32_t* __restrict__ vgraph, int32_t N,
                          VRec* __restrict__ vr, uint64_t* __restrict__ skey, uint32_t* __restrict__ sval) {
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int32_t v = N - 1 - i;  // descending id; the (stable) sort keeps this order inside a bucket
    int32_t d = colptr[v + 1] - colptr[v];
    VRec r; r.key = d; r.pqpos = -1; r.app_cnt = 0; r.app_chunk = -1;
    vr[v] = r;
    skey[i] = ((uint64_t)(uint32_t)vgraph[v] << 32) | (uint32_t)d;
    sval[i] = (uint32_t)v;
}

__global__ void k_bucket_bounds(const uint32_t* __restrict__ order, const VRec* __restrict__ vr, const int32_t* __restrict__ vgraph,
                                const GraphDesc* __restrict__ gd, int32_t N, int32_t* __restrict__ ocur, int32_t* __restrict__ oend,
                                int32_t* __restrict__ origpos) {
    int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    int32_t v = (int32_t)order[i];
    origpos[v] = i;
    int32_t g = vgraph[v], d = vr[v].key;
    int32_t b = gd[g].bucket_base + d;
    bool first = true, last = true;
    if (i > 0) { int32_t u = (int32_t)order[i - 1]; first = !(vgraph[u] == g && vr[u].key == d); }
    if (i < N - 1) { int32_t u = (int32_t)order[i + 1]; last = !(vgraph[u] == g && vr[u].key == d); }
    if (first) ocur[b] = i;
    if (last) oend[b] = i + 1;
}


}  // namespace rlap
