// rlap_gcnmath.h -- the scalar arithmetic of the GCN normalisation (rlap_snapshot_gcn_norm, rlap_gcn.hip).  Plain
// __host__ __device__ functions without any HIP dependency: tests/test_gcn_norm_cpu.py compiles this file with g++ and checks it
// against numpy.
//
// PyG's gcn_norm: deg[i] = sum of the weights of the entries whose target is i, dis[i] = deg[i]^-1/2 with 0 where deg[i] == 0, and
// the value of entry (i -> j, w) is dis[i] * w * dis[j], evaluated from the left.  Everything is float64; a float32 result is the
// float64 value rounded once (round to nearest even, what a C cast and numpy's astype do).  Square root, division and product are
// correctly rounded on the host and on the device (the library is built without fast-math and with contraction off), so the two
// give the same bits.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define RLAP_GCN_HD __host__ __device__ inline
#else
#define RLAP_GCN_HD inline
#endif

namespace rlap {
namespace gcnmath {

// deg^-1/2; 0 for deg == 0 (PyG's masked_fill of the infinity), and for anything that is not a positive number
RLAP_GCN_HD double dis(double deg) { return deg > 0.0 ? 1.0 / sqrt(deg) : 0.0; }

// the coefficient of entry (source i, target j, weight w)
RLAP_GCN_HD double value(double dis_i, double w, double dis_j) { return (dis_i * w) * dis_j; }

// a weight the normalisation accepts: finite and > 0 (false for NaN)
RLAP_GCN_HD bool weight_ok(double w) { return w > 0.0 && w < INFINITY; }

RLAP_GCN_HD float round32(double v) { return (float)v; }

}  // namespace gcnmath
}  // namespace rlap
