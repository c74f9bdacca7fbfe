// ekf_dense64_joint.hip -- the landmark front end of the dense64 handle for a WHOLE SCAN at once (gfx950, wave64): every
// reading is scored against the state the scan was taken at, one assignment is made, one stacked correction follows.
//   k_djt_terms     one thread per (reading, landmark) candidate: the body of k_dlm_terms (lm_store_terms), the reading from
//                   a device array instead of two kernel arguments
//   k_djt_argmin    one workgroup per reading: the lexicographic (score, index) minimum with NaNs skipped (lm_block_min) and
//                   the class of the reading -- MATCH, NEW or DROP -- by the rule of data_association (:293-330)
//   k_djt_resolve   one workgroup, one thread per reading: conflicts between MATCH readings, slots of the NEW ones, the final
//                   records, the header, the pair list, the stacked xb (initialize_landmark, :200-214) and W = sigma0 I
//   k_djt_operands  one workgroup: the stacked 2V x (3 + 2V) Jacobian, its column list, R = r_meas I and the innovation with
//                   the bearing wrapped, where the sparse correction reads its operands
// Small latency-bound launches: no floating-point atomics, no in-kernel waits, every reduction resolves ties to the lower
// index, so a run repeats in bits.  The model is measurement_terms of ekf_kernels.hpp through ekf_dense64_lm.hpp.
#include "ekf_dense64_lm.hpp"

namespace ekf {
namespace {

using namespace lm;

constexpr int kJointThreads = kDense64JointMaxReadings;   // k_djt_resolve: one thread per reading
constexpr int kOpThreads = 256;

__global__ __launch_bounds__(kLmThreads) void k_djt_terms(const double* __restrict__ state, const double* __restrict__ pose,
                                                          const double* __restrict__ xy, int n_readings, int first_lm,
                                                          int count, double r_meas, int* __restrict__ cols,
                                                          double* __restrict__ Hc, double* __restrict__ R,
                                                          double* __restrict__ nu) {
    const int c = blockIdx.x * kLmThreads + threadIdx.x, lane = threadIdx.x & 63;
    const double pv = pose[lane < 3 ? lane : 0];   // as k_dlm_terms: three lanes load, every lane is still active
    const double theta = lane_bcast(pv, 0), x = lane_bcast(pv, 1), y = lane_bcast(pv, 2);
    if (c == 0) {
        R[0] = r_meas; R[1] = 0.0; R[2] = 0.0; R[3] = r_meas;   // :172-175, shared by the candidates
    }
    if (c >= n_readings * count) return;   // (at most kDense64ScoreSparseMaxRows / 2 candidates a launch)
    const int j = c / count, i = c - j * count;
    const pair16 s = reinterpret_cast<const pair16*>(xy)[j];
    lm_store_terms(state, theta, x, y, s.x, s.y, first_lm + i, c, 0, cols, Hc, nu);
}

// block b: the scores nis [b][count] of one reading (count = known, 0: nothing scored and nis unread)
__global__ __launch_bounds__(kLmThreads) void k_djt_argmin(const double* __restrict__ nis, int count, double gate_new,
                                                           double gate_update, Dense64LmRecord* __restrict__ pre) {
    __shared__ Two sh[kLmThreads / 64];
    const Two t = lm_block_min(nis + (size_t)blockIdx.x * count, count, sh);
    if (threadIdx.x != 0) return;
    // :293-330 -- best = gate_new, win = known; ascending index with a strict <: the first of equal scores wins
    double best = gate_new;
    int win = count;
    if (t.b < best) {
        best = t.b;
        win = t.bi;
    }
    int kind = kDense64LmNew;                                             // NEW until k_djt_resolve has a slot for it
    if (win < count) kind = best < gate_update ? kDense64LmCorrect : 0;   // MATCH, or DROP
    Dense64LmRecord* r = pre + blockIdx.x;
    r->win = kind ? win : -1;
    r->kind = kind;
    r->best = best;
    r->runner = t.r;
    r->runner_idx = t.ri;
    r->pad = 0;
}

__global__ __launch_bounds__(kJointThreads) void k_djt_resolve(const Dense64LmRecord* __restrict__ pre, int J, int known,
                                                               int n_max, double gate_update, double sigma0,
                                                               const double* __restrict__ state,
                                                               const double* __restrict__ xy, int* __restrict__ head,
                                                               Dense64LmRecord* __restrict__ rec, int* __restrict__ pair_lm,
                                                               int* __restrict__ pair_j, double* __restrict__ xb,
                                                               double* __restrict__ W_full, double* __restrict__ W_last) {
    __shared__ int s_win[kJointThreads], s_kind[kJointThreads];
    __shared__ double s_best[kJointThreads];
    const int j = threadIdx.x;
    Dense64LmRecord r{-1, 0, 0.0, 0.0, 0, 0};
    if (j < J) r = pre[j];
    s_win[j] = r.win; s_kind[j] = r.kind; s_best[j] = r.best;
    __syncthreads();
    int win = r.win, kind = r.kind, rank = 0;
    if (kind == kDense64LmCorrect) {
        // among the MATCH readings that claim one landmark the smallest (best, j) keeps it
        for (int o = 0; o < J; o++)
            if (o != j && s_kind[o] == kDense64LmCorrect && s_win[o] == win && score_less(s_best[o], o, r.best, j)) kind = 0;
    } else if (kind == kDense64LmNew) {
        // the NEW readings take the slots known, known + 1, .. in ascending j while there is room
        for (int o = 0; o < j; o++) rank += s_kind[o] == kDense64LmNew;
        win = known + rank;
        if (win >= n_max) kind = 0;
        else if (0.0 < gate_update) kind |= kDense64LmCorrect;   // the gate sees 0 for a new landmark (:318-330)
    }
    if (kind == 0) win = -1;
    __syncthreads();
    s_kind[j] = kind;
    __syncthreads();
    int n_match = 0, n_new = 0, n_pairs = 0, before = 0;
    for (int o = 0; o < J; o++) {
        const int k = s_kind[o];
        n_new += (k & kDense64LmNew) != 0;
        n_match += k == kDense64LmCorrect;
        n_pairs += (k & kDense64LmCorrect) != 0;
        if (o < j) before += (k & kDense64LmCorrect) != 0;
    }
    if (j < J) {
        r.win = win;
        r.kind = kind;
        rec[j] = r;
        if (kind & kDense64LmCorrect) {   // the pairs of the correction in ascending j
            pair_lm[before] = win;
            pair_j[before] = j;
        }
        if (kind & kDense64LmNew) {
            const pair16 s = reinterpret_cast<const pair16*>(xy)[j];
            landmark_from_reading(s.x, s.y, state[0], state[1], state[2], xb[2 * rank], xb[2 * rank + 1]);   // at the pose on entry
        }
    }
    if (j == 0) {
        head[0] = n_match; head[1] = n_new; head[2] = n_pairs; head[3] = 0;
    }
    // W = sigma0 I for the initialisation's groups of 32 landmarks: r = 64 for a full group, r_last for the rest
    const int r_last = 2 * (n_new % kDense64JointInitGroup), r_full = 2 * kDense64JointInitGroup;
    if (n_new >= kDense64JointInitGroup)
        for (int e = j; e < r_full * r_full; e += kJointThreads) W_full[e] = e / r_full == e % r_full ? sigma0 : 0.0;
    for (int e = j; e < r_last * r_last; e += kJointThreads) W_last[e] = e / r_last == e % r_last ? sigma0 : 0.0;
}

// pair v: landmark lm [v] and reading rj [v] (v itself when rj is null) of xy.  m = 2 V rows, s = 3 + 2 V listed columns:
// cols = {0, 1, 2, 3 + 2 i0, 4 + 2 i0, 3 + 2 i1, ..}, rows 2 v and 2 v + 1 of Hc hold the reference's Hj (:158-166) at the
// local columns 0 .. 2 and 3 + 2 v, 4 + 2 v and zero elsewhere, nu has its bearing wrapped (:183), R = r_meas I
__global__ __launch_bounds__(kOpThreads) void k_djt_operands(const double* __restrict__ state, const double* __restrict__ xy,
                                                             const int* __restrict__ lm, const int* __restrict__ rj, int V,
                                                             double r_meas, int* __restrict__ cols, double* __restrict__ Hc,
                                                             double* __restrict__ R, double* __restrict__ nu) {
    const int tid = threadIdx.x, m = 2 * V, s = 3 + 2 * V;
    for (int e = tid; e < m * s; e += kOpThreads) Hc[e] = 0.0;
    for (int e = tid; e < m * m; e += kOpThreads) R[e] = e / m == e % m ? r_meas : 0.0;
    if (tid < 3) cols[tid] = tid;
    __syncthreads();
    if (tid >= V) return;
    const int i = lm[tid], j = rj ? rj[tid] : tid;
    const pair8 t = *reinterpret_cast<const pair8*>(state + 3 + 2 * i);
    const pair16 z = reinterpret_cast<const pair16*>(xy)[j];
    MeasTerms mt;
    measurement_terms(t.x, t.y, z.x, z.y, state[0], state[1], state[2], mt);
#pragma unroll
    for (int a = 0; a < 2; a++) {
        double* h = Hc + (size_t)(2 * tid + a) * s;
        h[0] = mt.H[a][0]; h[1] = mt.H[a][1]; h[2] = mt.H[a][2];
        h[3 + 2 * tid] = mt.H[a][3];
        h[4 + 2 * tid] = mt.H[a][4];
    }
    nu[2 * tid] = mt.z0 - mt.zh0;
    nu[2 * tid + 1] = normalize_angle(mt.z1 - mt.zh1);
    cols[3 + 2 * tid] = 3 + 2 * i;
    cols[4 + 2 * tid] = 4 + 2 * i;
}

}  // namespace

void launch_dense64_joint_terms(const double* state, const double* pose, const double* xy, int n_readings, int first_lm,
                                int count, double r_meas, int* cols, double* Hc, double* R, double* nu, hipStream_t st) {
    const int total = n_readings * count;
    hipLaunchKernelGGL(k_djt_terms, dim3((total + kLmThreads - 1) / kLmThreads), dim3(kLmThreads), 0, st, state, pose, xy,
                       n_readings, first_lm, count, r_meas, cols, Hc, R, nu);
}

void launch_dense64_joint_argmin(const double* nis, int n_readings, int count, double gate_new, double gate_update,
                                 Dense64LmRecord* pre, hipStream_t st) {
    hipLaunchKernelGGL(k_djt_argmin, dim3(n_readings), dim3(kLmThreads), 0, st, nis, count, gate_new, gate_update, pre);
}

void launch_dense64_joint_resolve(const Dense64LmRecord* pre, int J, int known, int n_max, double gate_update, double sigma0,
                                  const double* state, const double* xy, int* head, Dense64LmRecord* rec, int* pair_lm,
                                  int* pair_j, double* xb, double* W_full, double* W_last, hipStream_t st) {
    hipLaunchKernelGGL(k_djt_resolve, dim3(1), dim3(kJointThreads), 0, st, pre, J, known, n_max, gate_update, sigma0, state,
                       xy, head, rec, pair_lm, pair_j, xb, W_full, W_last);
}

void launch_dense64_joint_operands(const double* state, const double* xy, const int* lm, const int* rj, int V, double r_meas,
                                   int* cols, double* Hc, double* R, double* nu, hipStream_t st) {
    hipLaunchKernelGGL(k_djt_operands, dim3(1), dim3(kOpThreads), 0, st, state, xy, lm, rj, V, r_meas, cols, Hc, R, nu);
}

}  // namespace ekf
