// rlap_bitrank.h -- rank arithmetic on a bitmap of node ids (rlap_snapshot_subgraph, rlap_subgraph.hip).  Plain
// __host__ __device__ functions without any HIP dependency: tests/test_subgraph_cpu.py compiles this file with g++ and checks it
// against numpy.
//
// A node set is a bitmap: bit x of the call is bit (x & 63) of words[x >> 6].  scan[k] is the number of set bits in words[0 .. k),
// an exclusive scan of the words' population counts, so the number of set bits in front of bit x is
//     before(x) = scan[x >> 6] + popcount(words[x >> 6] & ((1 << (x & 63)) - 1))
// and the compact id of x inside a range that starts at bit lo (lo need not lie on the word grid) is before(x) - before(lo): the
// rank of x among the sorted set bits of the range.  The kernels keep word and scan entry of a position side by side (Rank): a
// label costs one gather, not two.  The table holds one entry more than the bitmap has words (the last word is zero, the last scan
// entry the total), so before(x) is defined for x = the number of bits as well.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RLAP_BR_HD __host__ __device__ inline
#else
#define RLAP_BR_HD inline
#endif

namespace rlap {
namespace bitrank {

RLAP_BR_HD int popc(uint64_t w) { return __builtin_popcountll(w); }

// words of a bitmap of `bits` bits, without the extra closing word
RLAP_BR_HD int64_t words_for(int64_t bits) { return (bits + 63) >> 6; }

// the bits of a word in front of bit x
RLAP_BR_HD uint64_t below(int64_t x) { return ((uint64_t)1 << (x & 63)) - 1; }

// a word and its scan entry side by side, so that one 16-byte load gives both
struct alignas(16) Rank { uint64_t word; int64_t scan; };

RLAP_BR_HD bool test(Rank e, int64_t x) { return (e.word >> (x & 63)) & 1; }
RLAP_BR_HD int64_t before(Rank e, int64_t x) { return e.scan + popc(e.word & below(x)); }

RLAP_BR_HD bool test(const Rank* r, int64_t x) { return test(r[x >> 6], x); }
RLAP_BR_HD int64_t before(const Rank* r, int64_t x) { return before(r[x >> 6], x); }

// rank of bit x among the set bits of [lo, ...), lo <= x
RLAP_BR_HD int64_t label(const Rank* r, int64_t lo, int64_t x) { return before(r, x) - before(r, lo); }

}  // namespace bitrank
}  // namespace rlap
