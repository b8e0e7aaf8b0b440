// The 16-slot shape of the degree order's round kernel on the CPU: host_mirror.cc's batch driver instantiated with CandT<16> and
// 256 candidates per round (tests/test_narrow_mirror.py).  Columns longer than 16 slots cut the round in front of them and, at the
// head of a round, take the driver's single-vertex path -- the device hands over to the 32-slot kernel there instead, which rests on
// the same property: every round commits a prefix of the sequential order.
#include "host_mirror.cc"

extern "C" int mirror_approx_chol_batch_narrow(const int64_t* row, const int64_t* col, const double* w, int64_t E, int64_t n, int64_t t,
                                               int o_v, int o_n, const int64_t* perm, uint64_t shuffle_seed, int32_t pool_slots, int32_t Bsz,
                                               double** out, int64_t* out_rows, int64_t* order_out, int64_t* stats_out) {
    static_assert(sizeof(CandT<16>) == 472, "256 records of the 16-slot shape: 120,832 bytes of LDS");
    return mirror_batch_impl<16>(row, col, w, E, n, t, o_v, o_n, perm, shuffle_seed, pool_slots, Bsz, out, out_rows, order_out, stats_out);
}
