// ekf_dense64_rot2.hpp -- device only: the 2 x 2 block G applied to a 2 x 2 block of Sigma from both sides, as step 1 of
// include/ekfslam.h's ekf_dense64_map_congruence defines it operation by operation.  Shared by the frame pass
// (ekf_dense64_frame.hip, in place) and the join pass (ekf_dense64_join.hip, out of place).
#pragma once
#include <hip/hip_runtime.h>

namespace ekf {
namespace rot2 {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef f64x2 f64x2u __attribute__((aligned(8)));   // a pair starts on an odd index: 8-byte aligned only

// (b0, b1) times one row of G: fl(fma(g1, b1, fl(g0 b0))).  The product from the left (G B, down a column of B) and the one
// from the right (B G^T, along a row of B) are this same expression.
__device__ __forceinline__ double one_sided(double g0, double g1, double b0, double b1) { return fma(g1, b1, g0 * b0); }

// Z = (G B) G^T for the block B = [a; b] (two rows of two)
__device__ __forceinline__ void both_sided(const double (&G)[4], f64x2 a, f64x2 b, f64x2* za, f64x2* zb) {
    const double y00 = one_sided(G[0], G[1], a[0], b[0]), y01 = one_sided(G[0], G[1], a[1], b[1]);
    const double y10 = one_sided(G[2], G[3], a[0], b[0]), y11 = one_sided(G[2], G[3], a[1], b[1]);
    *za = f64x2{one_sided(G[0], G[1], y00, y01), one_sided(G[2], G[3], y00, y01)};
    *zb = f64x2{one_sided(G[0], G[1], y10, y11), one_sided(G[2], G[3], y10, y11)};
}

}  // namespace rot2
}  // namespace ekf
