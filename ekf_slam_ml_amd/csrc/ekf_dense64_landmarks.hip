// ekf_dense64_landmarks.hip -- the reference's range-bearing landmark model and its decision rule on the dense64 handle's
// own state (gfx950, wave64): what a caller of the model-free sparse calls would otherwise compute on the host between them.
//   k_dlm_terms   one thread per candidate landmark: cols, Hc, nu (measurement_terms of ekf_kernels.hpp) and the shared R,
//                 written where k_dsp_score (or, with count = 1 and the wrapped innovation, the sparse correction) reads them;
//                 the pose through a pointer of its own (the state, or the snapshot of ekf_dense64_measure_landmarks)
//   k_dlm_decide  one workgroup: the lexicographic (score, index) minimum of the scores with NaNs skipped, the rule of
//                 data_association (:293-330), the inverse sensor model of a new landmark (:200-214), a 32-byte record
//   k_dlm_wrap    state[0] = normalize_angle(state[0]) (:187 / :385), stored unconditionally unless the correction refused
// No floating-point atomics, no LDS in k_dlm_terms; the model itself is ekf_kernels.hpp's, not a second copy, and what the
// joint form of the front end (ekf_dense64_joint.hip) needs of these kernels' bodies comes from ekf_dense64_lm.hpp.
#include "ekf_dense64_lm.hpp"

namespace ekf {
namespace {

using namespace lm;   // the pieces shared with ekf_dense64_joint.hip

__global__ __launch_bounds__(kLmThreads) void k_dlm_terms(const double* __restrict__ state,
                                                          const double* __restrict__ pose, double sx, double sy,
                                                          int first_lm, int count, int wrap, double r_meas,
                                                          int* __restrict__ cols, double* __restrict__ Hc,
                                                          double* __restrict__ R, double* __restrict__ nu) {
    const int j = blockIdx.x * kLmThreads + threadIdx.x, lane = threadIdx.x & 63;
    // the pose -- the state's own (data_association re-reads it per reading, :331-333) or the slot measurement() captured
    // it in (:109-111); the landmarks always come from the state.  Three lanes load it, the wave takes it through the scalar
    // file (every lane is still active here)
    const double pv = pose[lane < 3 ? lane : 0];
    const double theta = lane_bcast(pv, 0), x = lane_bcast(pv, 1), y = lane_bcast(pv, 2);
    if (j == 0) {
        R[0] = r_meas; R[1] = 0.0; R[2] = 0.0; R[3] = r_meas;   // :172-175, shared by the candidates
    }
    if (j >= count) return;
    lm_store_terms(state, theta, x, y, sx, sy, first_lm + j, j, wrap, cols, Hc, nu);
}

__global__ __launch_bounds__(kLmThreads) void k_dlm_decide(const double* __restrict__ nis, int count, int known, int n_max,
                                                           double gate_new, double gate_update, double sigma0,
                                                           const double* __restrict__ state, double sx, double sy,
                                                           Dense64LmRecord* __restrict__ rec, double* __restrict__ W,
                                                           double* __restrict__ xb) {
    __shared__ Two sh[kLmThreads / 64];
    const Two t = lm_block_min(nis, count, sh);
    if (threadIdx.x != 0) return;
    // :293-330 -- best = gate_new, win = known; ascending index with a strict <: the first of equal scores wins
    double best = gate_new;
    int win = known;
    if (t.b < best) {
        best = t.b;
        win = t.bi;
    }
    int kind = 0;
    double gate = best;
    if (win == known) {
        if (known < n_max) {   // :318-327 -- a new landmark; initialize_landmark (:200-214)
            landmark_from_reading(sx, sy, state[0], state[1], state[2], xb[0], xb[1]);
            W[0] = sigma0; W[1] = 0.0; W[2] = 0.0; W[3] = sigma0;
            kind = kDense64LmNew;
            gate = 0.0;
        } else {
            win = -1;   // a full map and nothing under the gate: dropped
        }
    }
    if (win >= 0 && gate < gate_update) kind |= kDense64LmCorrect;   // :330
    if (kind == 0) win = -1;
    rec->win = win;
    rec->kind = kind;
    rec->best = best;
    rec->runner = t.r;   // the second-smallest score and its candidate (+inf, INT_MAX with fewer than two scored)
    rec->runner_idx = t.ri;
    rec->pad = 0;
}

__global__ void k_dlm_wrap(double* __restrict__ state, const int* __restrict__ verdict) {
    if (threadIdx.x == 0 && *verdict == 0) state[0] = normalize_angle(state[0]);
}

}  // namespace

void launch_dense64_lm_terms(const double* state, const double* pose, double sx, double sy, int first_lm, int count,
                             int wrap, double r_meas, int* cols, double* Hc, double* R, double* nu, hipStream_t st) {
    hipLaunchKernelGGL(k_dlm_terms, dim3((count + kLmThreads - 1) / kLmThreads), dim3(kLmThreads), 0, st, state, pose, sx,
                       sy, first_lm, count, wrap, r_meas, cols, Hc, R, nu);
}

void launch_dense64_lm_decide(const double* nis, int count, int known, int n_max, double gate_new, double gate_update,
                              double sigma0, const double* state, double sx, double sy, Dense64LmRecord* rec, double* W,
                              double* xb, hipStream_t st) {
    hipLaunchKernelGGL(k_dlm_decide, dim3(1), dim3(kLmThreads), 0, st, nis, count, known, n_max, gate_new, gate_update,
                       sigma0, state, sx, sy, rec, W, xb);
}

void launch_dense64_lm_wrap(double* state, const int* verdict, hipStream_t st) {
    hipLaunchKernelGGL(k_dlm_wrap, dim3(1), dim3(64), 0, st, state, verdict);
}

}  // namespace ekf
