// rlap_squeeze.h -- the squeeze pass of the degree order (rlap_squeeze.hip): between two launches of the 16-slot round kernel every
// surviving column is rewritten, on all compute units, into the other entry arena as a plain CSR segment of its live entries
// (rlap_core.h::squeeze_entry is the rule).  A column's extent then equals its live count again, and the 16-slot kernel, which stops
// at the first column of more than 16 SLOTS, carries on until one has more than 16 live entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rlap_core.h"

namespace rlap {

constexpr int SQ_SHORT = 64;   // columns of up to this many slots take one thread each, longer ones (hubs, chunk chains) a wave

// Buffers of a call that squeezes (carved from the arena only then): the second arena, and the pass's own arrays.
struct SqueezeBufs {
    int passes;              // squeezes the schedule runs (SQUEEZE_PASSES; 0: none)
    Slot* e2;                // [slot_cap] the second entry arena (the passes alternate between the call's first one and this)
    int32_t* colptr2;        // [N + 1] ... and its column pointers
    int32_t* rank;           // [slot_cap] traversal rank of every live entry within its column
    int32_t* cnt;            // [N + 1] live entries per column (cnt[N] = 0: the scan's last element is the total)
    int32_t* longlist;       // [N] columns of more than SQ_SHORT slots
    int32_t* nlong;          // [1]
    int32_t* marks;          // [passes * G] graph g's narrow_rounds when pass p ran (what n_squeezes is counted from)
    const int32_t* vgraph;   // [N]
    void* scan_tmp; size_t scan_tmp_bytes;   // temporary storage of the prefix sum
    int32_t N;
};

// temporary storage the pass's prefix sum over N + 1 counts asks for
int squeeze_scan_tmp_bytes(int64_t N, size_t* bytes);

// One pass on `stream`, no host synchronisation: rank -> scan -> copy -> epilogue.  Reads the columns of A (A.e, A.colptr, A.vr),
// writes e_dst / colptr_dst, resets every vertex's appended entries, restarts the pool behind the new segments and clears each
// graph's pool reservation and `narrow` flag, so that the next launch of the 16-slot kernel tries again.  Rejected input (in_flags,
// in_acc: the round kernel's tests) and graphs with a non-zero status get empty columns: nothing of theirs is copied, and nothing
// downstream finds an entry to read.  Returns a hipError_t as int.
int launch_squeeze(hipStream_t stream, const Arrays& A, const SqueezeBufs& Q, int pass, Slot* e_dst, int32_t* colptr_dst, GraphDesc* gd, int32_t G,
                   const int32_t* in_flags, const double* in_acc);

}  // namespace rlap
