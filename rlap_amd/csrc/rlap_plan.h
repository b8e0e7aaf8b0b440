// rlap_plan.h -- propagation plans (rlap_snapshot_plan_build / _plan_propagate).  Two parts:
//   1. the layout rules of a plan as plain __host__ __device__ functions without any HIP dependency: tests/csrc/plan_mirror.cc
//      compiles them with g++ and checks them against a Python construction; the kernels of rlap_plan.hip read the same functions;
//   2. (HIP only) the interface between rlap_plan.hip, which holds the kernels and their orchestration, and the C ABI in
//      rlap_api.hip, which owns the handle, its lock and its arena.
// A plan holds every list of the product y = A^ x of rlap_snapshot_propagate, per direction: the entries that stay, in the order
// rlap_spmm.h sums them, as 16-byte records; off[slot], slot = layer * N + id, is the first record of that id's list and
// off[slot + 1] the end; the lists longer than spmm::CHUNK have their chunks numbered in slot order, and the directory names the
// (slot, chunk of the list) of every number.  The summation order itself stays in rlap_spmm.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rlap_spmm.h"

namespace rlap {
namespace plan {

constexpr int FORWARD = 0, TRANSPOSED = 1;
constexpr int32_t MAGIC = 0x504c414e;   // rlap_plan_desc.magic of a successful build

// one entry of a list: its coefficient and the id whose row of x it takes (16 bytes, one load)
struct alignas(16) Record { double c; int32_t id; int32_t zero; };
// one chunk of a long list: the list's slot and the chunk's number within it
struct alignas(16) ChunkRef { int64_t slot; int64_t k; };

RLAP_SPMM_HD int64_t align_up(int64_t v) { return (v + 255) & ~(int64_t)255; }

// the slot of (layer, id): lists, offsets and loop coefficients are indexed by it
RLAP_SPMM_HD int64_t slot_of(int64_t layer, int64_t N, int64_t id) { return layer * N + id; }

// chunks of a list of `kept` entries that the directory lists: none for a list of one chunk (it is summed by its own group)
RLAP_SPMM_HD int64_t dir_chunks(int64_t kept) { return kept > spmm::CHUNK ? spmm::num_chunks(kept) : 0; }

// chunks the directory of a direction can need: a list of n > CHUNK entries has at most 2 n / CHUNK chunks, and the lists of a
// direction share the m rows
RLAP_SPMM_HD int64_t dir_cap(int64_t m) { return m > spmm::CHUNK ? 2 * m / spmm::CHUNK + 2 : 0; }

// an entry's place in its list.  Without dropped loop rows: its distance from the list's first position (of the rows, forward; of
// the rows sorted by source, transposed).  With dropped loop rows: the entries in front of it that stay -- is_loop(k) says
// whether position k of the list is a loop row; the list is walked, counting.
RLAP_SPMM_HD int64_t place_plain(int64_t first, int64_t pos) { return pos - first; }
template <class IsLoop>
RLAP_SPMM_HD int64_t place_counting(int64_t k, IsLoop is_loop) {
    int64_t kept = 0;
    for (int64_t j = 0; j < k; ++j) kept += is_loop(j) ? 0 : 1;
    return kept;
}

// where the record of an entry goes, or -1 when the place lies outside the list's records [off0, off1) (a malformed input)
RLAP_SPMM_HD int64_t record_index(int64_t off0, int64_t off1, int64_t place) {
    return (place >= 0 && off0 >= 0 && off0 + place < off1) ? off0 + place : -1;
}

// the directory entries of one list: first = chunks of the lists in front of it (in slot order); put(q, ChunkRef) writes number q
template <class Put>
RLAP_SPMM_HD void dir_write(int64_t slot, int64_t kept, int64_t first, int64_t cap, Put put) {
    const int64_t nc = dir_chunks(kept);
    for (int64_t k = 0; k < nc && first + k < cap; ++k) put(first + k, ChunkRef{slot, k});
}

// the first directory number of `slot`'s list: the first q in [0, chunks) whose slot is not below it (the directory is in slot
// order); slot_at(q) reads one
template <class SlotAt>
RLAP_SPMM_HD int64_t dir_first(int64_t chunks, int64_t slot, SlotAt slot_at) {
    int64_t lo = 0, hi = chunks;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (slot_at(mid) < slot) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// byte offsets of the parts of a plan buffer (every part 256-byte aligned; -1: the part is not there).  The records come last,
// the transposed ones behind the forward ones, so that what a build does not fill is the buffer's tail.
struct Layout {
    int64_t loop;                 // double[slots], with self loops
    int64_t off[2];               // int64[slots + 1]
    int64_t dir[2];               // ChunkRef[dir_cap(m)]
    int64_t rec[2];               // Record[m]
    int64_t bytes;
};
RLAP_SPMM_HD Layout layout(int64_t m, int64_t slots, bool loops, bool forward, bool transposed) {
    Layout L;
    int64_t at = 0;
    const bool has[2] = {forward, transposed};
    L.loop = -1;
    if (loops) { L.loop = at; at = align_up(at + 8 * slots); }
    for (int d = 0; d < 2; ++d) {
        L.off[d] = -1;
        if (has[d]) { L.off[d] = at; at = align_up(at + 8 * (slots + 1)); }
    }
    for (int d = 0; d < 2; ++d) {
        L.dir[d] = -1;
        if (has[d]) { L.dir[d] = at; at = align_up(at + (int64_t)sizeof(ChunkRef) * dir_cap(m)); }
    }
    for (int d = 0; d < 2; ++d) {
        L.rec[d] = -1;
        if (has[d]) { L.rec[d] = at; at = align_up(at + (int64_t)sizeof(Record) * m); }
    }
    L.bytes = at > 0 ? at : 256;
    return L;
}

}  // namespace plan
}  // namespace rlap

#if defined(__HIPCC__) || defined(__HIP__)
#include "rlap_snapshot.h"

namespace rlap {

struct SnapshotPlanArgs {
    SnapshotSeg seg;
    int flags;                                // RLAP_GCN_WEIGHTED / SELF_LOOPS / NORMALIZE, RLAP_PLAN_* resolved (include/rlap_hip.h)
    double fill;                              // weight of an added self loop
    void* plan; size_t plan_bytes;            // the caller's buffer
};

struct SnapshotPlanReport {
    int64_t entries, blocks, loops_removed;
    int64_t dir_entries[2], dir_chunks[2], chunked[2];   // per direction: records, chunks of the long lists, long lists
    int32_t host_syncs;
};

struct PlanUseArgs {
    const void* plan; const rlap_plan_desc* desc;
    int flags;                                // RLAP_SPMM_*
    const void* x; int64_t F; void* y;
    int64_t part_limit;                       // test hook: chunk sums the call may keep (negative: the budget of rlap_plan.hip)
};

// bytes of the plan buffer (an upper bound); arena bytes of the build
size_t snapshot_plan_buffer_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int flags);
size_t snapshot_plan_build_bytes(int64_t m, int64_t S, int64_t G, int64_t N, int flags);
// the build on `stream`, with `ws` as its scratch; fills *desc on success; returns an RLAP_* status
int snapshot_plan_build_run(hipStream_t stream, void* ws, size_t ws_bytes, const SnapshotPlanArgs& a, rlap_plan_desc* desc,
                            SnapshotPlanReport* rep);
// arena bytes of a planned call, and the call (no host synchronisation)
size_t snapshot_plan_use_bytes(const rlap_plan_desc& d, int64_t F, int flags, int64_t part_limit);
int snapshot_plan_use_run(hipStream_t stream, void* ws, size_t ws_bytes, const PlanUseArgs& a);

}  // namespace rlap
#endif
