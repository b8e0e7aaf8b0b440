// Host mirror of the propagation's summation order: rlap_amd/csrc/rlap_spmm.h -- the very header rlap_spmm.hip includes -- compiled
// with g++ -ffp-contract=off.  tests/test_propagate_cpu.py checks it against numpy; tests/test_gpu_propagate.py feeds it the
// coefficients of ops.snapshot_gcn_norm and compares the device's result bit for bit.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "rlap_readout.h"
#include "rlap_spmm.h"

extern "C" {

// the readout's dispatch rule (rlap_readout.h), for the regime accounting of tests/test_gpu_readout_regimes.py: out = vec, lanes, lg, ftiles
void readout_dispatch(int64_t F, int elem_bytes, int aligned16, int64_t* out) {
    const rlap::readout::Dispatch d = rlap::readout::dispatch(F, elem_bytes, aligned16 != 0);
    out[0] = d.vec ? 1 : 0;
    out[1] = d.lanes;
    out[2] = d.lg;
    out[3] = d.ftiles;
}

int spmm_chunk() { return rlap::spmm::CHUNK; }

// one element: the list's n terms c[e] * x[e], then (has_loop) c_loop * x_loop
double spmm_list(int64_t n, const double* c, const double* x, int has_loop, double c_loop, double x_loop) {
    return rlap::spmm::list_sum(n, [&](int64_t e) { return c[e]; }, [&](int64_t e) { return x[e]; }, has_loop != 0, c_loop, x_loop);
}

// A list of E entries (src -> dst, val) over ids [0, N), x (N, F) row-major -> y (N, F): y[j] sums the entries whose target is j
// (transpose: whose source is j, taking x[target]) in their order in the list.  With `loops` the entries with src == dst are the
// loop terms (one per id at most, wherever it stands in the list: it is added last); without, they are entries like the others.
void spmm_entries(int64_t E, const int64_t* src, const int64_t* dst, const double* val, int64_t N, int64_t F, const double* x,
                  int loops, int transpose, double* y) {
    std::vector<std::vector<int64_t>> lists((size_t)N);
    std::vector<int64_t> loop((size_t)N, -1);
    for (int64_t e = 0; e < E; ++e) {
        if (loops && src[e] == dst[e]) loop[(size_t)src[e]] = e;
        else lists[(size_t)(transpose ? src[e] : dst[e])].push_back(e);
    }
    for (int64_t j = 0; j < N; ++j) {
        const std::vector<int64_t>& l = lists[(size_t)j];
        const int64_t n = (int64_t)l.size(), le = loop[(size_t)j];
        const int64_t* from = transpose ? dst : src;
        for (int64_t f = 0; f < F; ++f) {
            auto coef = [&](int64_t k) { const int64_t e = l.at((size_t)k); return val[e]; };
            auto feat = [&](int64_t k) { const int64_t e = l.at((size_t)k); return x[from[e] * F + f]; };
            y[j * F + f] = rlap::spmm::list_sum(n, coef, feat, le >= 0, le >= 0 ? val[le] : 0.0, x[j * F + f]);
        }
    }
}

}  // extern "C"
