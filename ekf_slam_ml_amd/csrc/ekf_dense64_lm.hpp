// ekf_dense64_lm.hpp -- the device pieces the landmark front end (ekf_dense64_landmarks.hip, one reading at a time) and its
// joint form (ekf_dense64_joint.hip, a whole scan at once) share, so that neither holds a second copy:
//   lm_store_terms   the operands of ONE (reading, landmark) candidate where k_dsp_score reads them
//   Two, lm_insert, lm_merge, lm_block_min   the two smallest (score, index) pairs of a list, ties to the lower index
//                    (score_less of ekf_assoc.hpp)
// The model itself is measurement_terms and landmark_from_reading of ekf_kernels.hpp.
#pragma once
#include "ekf_assoc.hpp"
#include "ekf_dense.hpp"

namespace ekf {
namespace lm {

constexpr int kLmThreads = 256;

// two doubles that sit on an 8-byte boundary only (landmark i starts at state + 3 + 2 i): one 16-byte access
typedef double pair8 __attribute__((ext_vector_type(2), aligned(8)));
typedef double pair16 __attribute__((ext_vector_type(2)));

// candidate c of a launch: the reading (sx, sy) against landmark i of `state`, at the pose (theta, x, y).  cols [c][5],
// Hc [c][2][5] and nu [c][2] on 16-byte boundaries; the bearing of nu raw (the score's, :269) or wrapped (the correction's,
// :183)
__device__ __forceinline__ void lm_store_terms(const double* __restrict__ state, double theta, double x, double y, double sx,
                                               double sy, int i, int c, int wrap, int* __restrict__ cols,
                                               double* __restrict__ Hc, double* __restrict__ nu) {
    const pair8 t = *reinterpret_cast<const pair8*>(state + 3 + 2 * i);
    MeasTerms m;
    measurement_terms(t.x, t.y, sx, sy, theta, x, y, m);
    const double d1 = m.z1 - m.zh1;   // raw for the score (:269), wrapped for the correction (:183)
    pair16* h = reinterpret_cast<pair16*>(Hc + (size_t)c * 10);   // 80 bytes per candidate on a 16-byte base
    h[0] = pair16{m.H[0][0], m.H[0][1]};
    h[1] = pair16{m.H[0][2], m.H[0][3]};
    h[2] = pair16{m.H[0][4], m.H[1][0]};
    h[3] = pair16{m.H[1][1], m.H[1][2]};
    h[4] = pair16{m.H[1][3], m.H[1][4]};
    reinterpret_cast<pair16*>(nu)[c] = pair16{m.z0 - m.zh0, wrap ? normalize_angle(d1) : d1};
    int* cc = cols + (size_t)c * 5;
    cc[0] = 0; cc[1] = 1; cc[2] = 2; cc[3] = 3 + 2 * i; cc[4] = 4 + 2 * i;
}

// the two smallest (score, index) pairs seen so far, in the order "smaller score, then smaller index"
struct Two {
    double b, r;
    int bi, ri;
};
__device__ __forceinline__ void lm_insert(Two& t, double v, int vi) {
    if (score_less(v, vi, t.b, t.bi)) {
        t.r = t.b; t.ri = t.bi; t.b = v; t.bi = vi;
    } else if (score_less(v, vi, t.r, t.ri)) {
        t.r = v; t.ri = vi;
    }
}
// the union of two disjoint sets (the sentinels excepted, which are equal): the same result in either order
__device__ __forceinline__ void lm_merge(Two& t, const Two& o) {
    lm_insert(t, o.b, o.bi);
    lm_insert(t, o.r, o.ri);
}

// One workgroup of kLmThreads: the two smallest of nis [count] with NaNs skipped (a NaN -- a flagged candidate -- never
// wins and disturbs nobody); with `bounded`, of the pairs strictly above (after, after_i) in that order only.  The result is
// thread 0's; sh: one Two per wave.  Every thread of the block calls it, and a second call waits for a barrier behind the
// first (thread 0 reads sh).
__device__ __forceinline__ Two lm_block_min_after(const double* __restrict__ nis, int count, Two* sh, bool bounded,
                                                  double after, int after_i) {
    const int tid = threadIdx.x;
    const double inf = __builtin_huge_val();
    Two t{inf, inf, 0x7fffffff, 0x7fffffff};
    for (int j = tid; j < count; j += kLmThreads) {
        const double v = nis[j];
        if (v == v && (!bounded || score_less(after, after_i, v, j))) lm_insert(t, v, j);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        Two o;
        o.b = __shfl_xor(t.b, off, 64);
        o.bi = __shfl_xor(t.bi, off, 64);
        o.r = __shfl_xor(t.r, off, 64);
        o.ri = __shfl_xor(t.ri, off, 64);
        lm_merge(t, o);
    }
    if ((tid & 63) == 0) sh[tid >> 6] = t;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < kLmThreads / 64; w++) lm_merge(t, sh[w]);
    return t;
}
__device__ __forceinline__ Two lm_block_min(const double* __restrict__ nis, int count, Two* sh) {
    return lm_block_min_after(nis, count, sh, false, 0.0, 0);
}

}  // namespace lm
}  // namespace ekf
