// rlap_spmm.h -- the summation order of the GCN propagation (rlap_snapshot_propagate, rlap_spmm.hip).  Plain
// __host__ __device__ functions without any HIP dependency: tests/test_propagate_cpu.py compiles this file with g++ (through
// tests/csrc/spmm_mirror.cc) and checks it against numpy; the kernels read the same functions.
//
// One element of the result is the sum of a LIST of terms c_e * x_e -- the entries of one target (forward) or of one source
// (transposed) in their input order -- and of one optional loop term that comes last.  The order is part of the contract:
//   * every term is the float64 product c_e * x_e, rounded; every add is a float64 add, rounded; nothing is fused (the library and
//     the mirror are built with contraction off);
//   * the list is cut into chunks of CHUNK entries (the last one may be shorter; an empty list has no chunk); a chunk is summed
//     from 0 in list order;
//   * the chunk sums are added to 0 in chunk order (a list of up to CHUNK entries is one chunk: 0 + its sum);
//   * the loop term is added last.
// So the result depends on nothing but an entry's place in its list, whichever wave sums which chunk.  A float32 result is the
// float64 sum rounded once.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RLAP_SPMM_HD __host__ __device__ inline
#else
#define RLAP_SPMM_HD inline
#endif

namespace rlap {
namespace spmm {

constexpr int CHUNK = 256;   // entries of a list that one wave sums in a row

// chunks of a list of n entries, and the entries [chunk_begin(k), chunk_end(n, k)) of chunk k
RLAP_SPMM_HD int64_t num_chunks(int64_t n) { return n > 0 ? (n + CHUNK - 1) / CHUNK : 0; }
RLAP_SPMM_HD int64_t chunk_begin(int64_t k) { return k * CHUNK; }
RLAP_SPMM_HD int64_t chunk_end(int64_t n, int64_t k) { return (k + 1) * CHUNK < n ? (k + 1) * CHUNK : n; }

// acc + c * x: the product rounded, then the add rounded
RLAP_SPMM_HD double accumulate(double acc, double c, double x) {
    const double t = c * x;
    return acc + t;
}

// the sum of chunk k of a list: coef(e) and feat(e) give c_e and x_e of entry e of the list
template <class Coef, class Feat>
RLAP_SPMM_HD double chunk_sum(int64_t n, int64_t k, Coef coef, Feat feat) {
    double s = 0.0;
    for (int64_t e = chunk_begin(k); e < chunk_end(n, k); ++e) s = accumulate(s, coef(e), feat(e));
    return s;
}

// the whole rule: the list's n entries, then (has_loop) the loop term c_loop * x_loop
template <class Coef, class Feat>
RLAP_SPMM_HD double list_sum(int64_t n, Coef coef, Feat feat, bool has_loop, double c_loop, double x_loop) {
    double total = 0.0;
    for (int64_t k = 0; k < num_chunks(n); ++k) total = total + chunk_sum(n, k, coef, feat);
    if (has_loop) total = accumulate(total, c_loop, x_loop);
    return total;
}

}  // namespace spmm
}  // namespace rlap
