// ekf_assoc.hpp -- the decision step of data_association() (ekf_slam.cpp:293-330) on the device, ONCE: every kernel form
// (k_assoc_decide, k_assoc_reading, k_assoc_call, k_pool_step_unknown, the small-map body) takes the rule from here, so the
// forms cannot drift apart.  A kernel keeps what is its own: where the scores come from, where a new landmark's position
// is parked (landmark_from_reading of ekf_kernels.hpp writes it), what is published to the host.
//   score_take, score_less, wave_argmin,    the sequential scan's first strict minimum as a lexicographic (score, index)
//   block_argmin                            reduction: independent of the launch geometry; NaN scores never win
//   assoc_decision                          min_maha_idx, the new-landmark rule and the gate_update test
//   maha_quad, maha_score                   the score of one (reading, landmark) candidate (:217-276) from its 5 x 5 block
//   fold_pair                               one pending rank-2 pair taken off a 5 x 5 block (k_rank2's expression)
// Device code only.  Every expression keeps the order of the scalar reference restatement (-ffp-contract=off).
#pragma once
#include <climits>

#include "ekf_kernels.hpp"

namespace ekf {

// (score, index) order: the smaller score, then the lower index.  score_take is the step of every reduction:
// (d, i) <- (od, oi) where that is the smaller one; score_less is the same comparison without the assignment.
__device__ __forceinline__ bool score_take(double& d, int& i, double od, int oi) {
    if (od < d || (od == d && oi < i)) { d = od; i = oi; return true; }
    return false;
}
__device__ __forceinline__ bool score_less(double a, int ai, double b, int bi) { return score_take(b, bi, a, ai); }

// one wavefront: the minimum of its lanes' (d, i), valid in lane 0
__device__ __forceinline__ void wave_argmin(double& d, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_down(d, off, kWave);
        const int oi = __shfl_down(i, off, kWave);
        score_take(d, i, od, oi);
    }
}

// One workgroup, in two halves with the caller's barrier (and whatever it stamps there) in between: every thread calls
// block_argmin_stage, lane 0 of each wave leaves its minimum in sh_d / sh_i [waves]; behind the barrier thread 0 alone calls
// block_argmin_fold and holds the workgroup's minimum.
__device__ __forceinline__ void block_argmin_stage(double& d, int& i, double* sh_d, int* sh_i) {
    wave_argmin(d, i);
    if ((threadIdx.x & 63) == 0) { sh_d[threadIdx.x >> 6] = d; sh_i[threadIdx.x >> 6] = i; }
}
__device__ __forceinline__ void block_argmin_fold(double& d, int& i, const double* sh_d, const int* sh_i, int waves) {
    for (int w = 1; w < waves; w++) score_take(d, i, sh_d[w], sh_i[w]);
}
// ... and both around a barrier of its own: the result is thread 0's.  Every thread of the workgroup calls it.
__device__ __forceinline__ void block_argmin(double& d, int& i, double* sh_d, int* sh_i, int waves) {
    block_argmin_stage(d, i, sh_d, sh_i);
    __syncthreads();
    if (threadIdx.x == 0) block_argmin_fold(d, i, sh_d, sh_i, waves);
}

// What one reading leads to.  (rd, ri): the minimum of the scores of the M known landmarks below gate_new, or
// (gate_new, INT_MAX) when there is none (:293); n: the map's capacity.  Called by one thread; where is_new, the caller
// writes the position of landmark idx (landmark_from_reading, :318-327) -- the gate sees 0 for it.
struct AssocDecision {
    int idx;           // min_maha_idx (:294: known_count when nothing is under the gate)
    int known_count;   // M, or M + 1 behind a new landmark
    int is_new;
    int active;        // the reading corrects landmark idx
    double best;       // what the gate_update test saw
    __device__ __forceinline__ int lm() const { return active ? idx : -1; }
};
__device__ __forceinline__ AssocDecision assoc_decision(double rd, int ri, int M, int n, double gate_update) {
    AssocDecision a;
    a.idx = (ri == INT_MAX) ? M : ri;
    a.is_new = a.idx == M && a.idx < n;
    a.known_count = a.is_new ? M + 1 : M;
    a.best = a.is_new ? 0.0 : rd;
    // :330.  idx == n (map full, no match) can only pass the gate with non-reference parameters (gate_new < gate_update);
    // the reference would index out of bounds there.
    a.active = (a.best < gate_update) && a.idx < n;
    return a;
}

// nu^T S^-1 nu (:270-273)
__device__ __forceinline__ double maha_quad(const double Si[2][2], double v0, double v1) {
    const double t0 = v0 * Si[0][0] + v1 * Si[1][0];
    const double t1 = v0 * Si[0][1] + v1 * Si[1][1];
    return t0 * v0 + t1 * v1;
}

// The score of the candidate whose terms are m and whose block Sigma[c5, c5] is S55 (innovation_cov sums in the order of
// k_maha's shuffle folds).  Si and the innovation (v0, v1), its bearing NOT wrapped (:269), are left for a caller that
// keeps the winner's terms for the correction.
__device__ __forceinline__ double maha_score(const double S55[5][5], const MeasTerms& m, double r_meas, double Si[2][2],
                                             double& v0, double& v1) {
    double S[2][2];
    innovation_cov(S55, m.H, r_meas, S);
    inv2(S, Si);
    v0 = m.z0 - m.zh0;
    v1 = m.z1 - m.zh1;
    return maha_quad(Si, v0, v1);
}

// S55 <- S55 - (K_pair G_pair) at the block's five indices: kr[k] = (K(c5[k], 0), K(c5[k], 1)), gc[l] = (G(0, c5[l]), G(1, c5[l]))
__device__ __forceinline__ void fold_pair(double (&S55)[5][5], const double (&kr)[5][2], const double (&gc)[5][2]) {
#pragma unroll
    for (int k = 0; k < 5; k++)
#pragma unroll
        for (int l = 0; l < 5; l++) S55[k][l] = S55[k][l] - (kr[k][0] * gc[l][0] + kr[k][1] * gc[l][1]);
}

}  // namespace ekf
