// ekf_dense64_landmarks.hip -- the reference's range-bearing landmark model and its decision rule on the dense64 handle's
// own state (gfx950, wave64): what a caller of the model-free sparse calls would otherwise compute on the host between them.
//   k_dlm_terms   one thread per candidate landmark: cols, Hc, nu (measurement_terms of ekf_kernels.hpp) and the shared R,
//                 written where k_dsp_score (or, with count = 1 and the wrapped innovation, the sparse correction) reads them;
//                 the pose through a pointer of its own (the state, or the snapshot of ekf_dense64_measure_landmarks)
//   k_dlm_decide  one workgroup: the lexicographic (score, index) minimum of the scores with NaNs skipped, the rule of
//                 data_association (:293-330), the inverse sensor model of a new landmark (:200-214), a 32-byte record
//   k_dlm_wrap    state[0] = normalize_angle(state[0]) (:187 / :385), stored unconditionally unless the correction refused
// No floating-point atomics, no LDS in k_dlm_terms; the model itself is ekf_kernels.hpp's, not a second copy.
#include "ekf_dense.hpp"
#include "ekf_kernels.hpp"

namespace ekf {
namespace {

constexpr int kLmThreads = 256;

// two doubles that sit on an 8-byte boundary only (landmark i starts at state + 3 + 2 i): one 16-byte access
typedef double pair8 __attribute__((ext_vector_type(2), aligned(8)));
typedef double pair16 __attribute__((ext_vector_type(2)));

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
    const int i = first_lm + j;
    const pair8 t = *reinterpret_cast<const pair8*>(state + 3 + 2 * i);
    MeasTerms m;
    measurement_terms(t.x, t.y, sx, sy, theta, x, y, m);
    const double d1 = m.z1 - m.zh1;   // raw for the score (:269), wrapped for the correction (:183)
    pair16* h = reinterpret_cast<pair16*>(Hc + (size_t)j * 10);   // 80 bytes per candidate on a 16-byte base
    h[0] = pair16{m.H[0][0], m.H[0][1]};
    h[1] = pair16{m.H[0][2], m.H[0][3]};
    h[2] = pair16{m.H[0][4], m.H[1][0]};
    h[3] = pair16{m.H[1][1], m.H[1][2]};
    h[4] = pair16{m.H[1][3], m.H[1][4]};
    reinterpret_cast<pair16*>(nu)[j] = pair16{m.z0 - m.zh0, wrap ? normalize_angle(d1) : d1};
    int* c = cols + (size_t)j * 5;
    c[0] = 0; c[1] = 1; c[2] = 2; c[3] = 3 + 2 * i; c[4] = 4 + 2 * i;
}

// the two smallest (score, index) pairs seen so far, in the order "smaller score, then smaller index"
struct Two {
    double b, r;
    int bi, ri;
};
__device__ __forceinline__ bool lm_less(double a, int ai, double b, int bi) { return a < b || (a == b && ai < bi); }
__device__ __forceinline__ void lm_insert(Two& t, double v, int vi) {
    if (lm_less(v, vi, t.b, t.bi)) {
        t.r = t.b; t.ri = t.bi; t.b = v; t.bi = vi;
    } else if (lm_less(v, vi, t.r, t.ri)) {
        t.r = v; t.ri = vi;
    }
}
// the union of two disjoint sets (the sentinels excepted, which are equal): the same result in either order
__device__ __forceinline__ void lm_merge(Two& t, const Two& o) {
    lm_insert(t, o.b, o.bi);
    lm_insert(t, o.r, o.ri);
}

__global__ __launch_bounds__(kLmThreads) void k_dlm_decide(const double* __restrict__ nis, int count, int known, int n_max,
                                                           double gate_new, double gate_update, double sigma0,
                                                           const double* __restrict__ state, double sx, double sy,
                                                           Dense64LmRecord* __restrict__ rec, double* __restrict__ W,
                                                           double* __restrict__ xb) {
    __shared__ Two sh[kLmThreads / 64];
    const int tid = threadIdx.x;
    const double inf = __builtin_huge_val();
    Two t{inf, inf, 0x7fffffff, 0x7fffffff};
    for (int j = tid; j < count; j += kLmThreads) {
        const double v = nis[j];
        if (v == v) lm_insert(t, v, j);   // a NaN (a flagged candidate) never wins and disturbs nobody
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
    if (tid != 0) return;
    for (int w = 1; w < kLmThreads / 64; w++) lm_merge(t, sh[w]);
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
            const double theta = state[0], x = state[1], y = state[2];
            const double ri = sqrt(sx * sx + sy * sy);
            const double phii = atan2(sy, sx);
            xb[0] = x + ri * cos(phii + theta);
            xb[1] = y + ri * sin(phii + theta);
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
