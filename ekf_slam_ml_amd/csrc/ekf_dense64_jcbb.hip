// ekf_dense64_jcbb.hip -- the device half of the joint compatibility association of the dense fp64 handle (gfx950, wave64):
// the candidates of every reading of a scan, their operands, and the CROSS BLOCKS H_p Sigma H_q^T between different
// candidate pairings, which no other call produces.  The search over them is the host's (ekf_dense64_jcbb.hpp).
//   k_jc_select   one workgroup per reading over the scores the scoring launch left on the device: the up to C lowest
//                 (score, index) pairs with score < gate_ic in ascending lexicographic order, NaNs skipped, ties to the lower
//                 index.  Round c takes the two smallest pairs (lm_block_min_after) strictly above round c - 1's second, so
//                 the result is a function of the scores alone, not of the launch geometry.  Also best and is_new as
//                 k_djt_argmin defines them.
//   k_jc_terms    one workgroup: the offsets (an exclusive scan of the counts by one thread), the candidates numbered in
//                 ascending (reading, rank), and per candidate lm_store_terms at the pose on entry, bearing raw
//   k_jc_cross    one thread per (p, q) block, a workgroup per 16 x 16 tile: W[p][q] = Hc_p Sigma[cols_p, cols_q] Hc_q^T in
//                 the order of k_dsp_score (acc = +0; acc = fma(x_k, y_k, acc), k ascending; T' rounded to fp64 in between),
//                 p == q: + r_meas delta_ab by one plain addition -- so W[p][p] is that kernel's S bit for bit.  The tile's
//                 operands and the 3 x 3 pose block sit in LDS, the landmark parts of Sigma are gathered; Sigma is read as
//                 stored, never symmetrised.  P is read from the record k_jc_terms left: the tile slack is masked, nothing
//                 outside the live corner is read, nothing outside [P][P] is written.
// No atomics, no in-kernel waits, every loop bound a kernel argument or a constant: a run repeats in bits, and a block's
// bits depend on its two candidates alone.
#include "ekf_dense64_lm.hpp"

namespace ekf {
namespace {

using namespace lm;

constexpr int kJcTile = kDense64JcbbTile, kJcThreads = kJcTile * kJcTile;
constexpr int kJcMaxJ = kDense64JcbbMaxReadings, kJcMaxC = kDense64JcbbMaxCand, kJcMaxP = kJcMaxJ * kJcMaxC;
static_assert(kJcThreads == 256 && kJcMaxP <= kLmThreads, "one thread per block of a tile, one per candidate");

// block b: reading j0 + b, its scores nis [b][count]
__global__ __launch_bounds__(kLmThreads) void k_jc_select(const double* __restrict__ nis, int count, int j0, int C,
                                                          double gate_ic, double gate_new, int* __restrict__ cand_count,
                                                          int* __restrict__ cand_lm, double* __restrict__ cand_nis,
                                                          double* __restrict__ best, int* __restrict__ is_new) {
    __shared__ Two sh[kLmThreads / 64];
    __shared__ double s_after;
    __shared__ int s_after_i;
    const int j = j0 + blockIdx.x;
    const double* row = nis + (size_t)blockIdx.x * count;
    int n = 0;
    for (int c = 0; c < C; c += 2) {
        const Two t = lm_block_min_after(row, count, sh, c > 0, c > 0 ? s_after : 0.0, c > 0 ? s_after_i : 0);
        __syncthreads();   // every wave is done with sh and with the bound of this round
        if (threadIdx.x == 0) {
            if (c == 0) {   // best = gate_new unless something lies below it (k_djt_argmin)
                best[j] = t.b < gate_new ? t.b : gate_new;
                is_new[j] = t.b < gate_new ? 0 : 1;
            }
            if (t.b < gate_ic) {
                cand_lm[j * kJcMaxC + n] = t.bi;
                cand_nis[j * kJcMaxC + n] = t.b;
                n++;
            }
            if (c + 1 < C && t.r < gate_ic) {
                cand_lm[j * kJcMaxC + n] = t.ri;
                cand_nis[j * kJcMaxC + n] = t.r;
                n++;
            }
            s_after = t.r;
            s_after_i = t.ri;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        for (int c = n; c < kJcMaxC; c++) {
            cand_lm[j * kJcMaxC + c] = -1;
            cand_nis[j * kJcMaxC + c] = __builtin_huge_val();
        }
        cand_count[j] = n;
    }
}

// one workgroup of kJcMaxP threads; head [0] = P
__global__ __launch_bounds__(kJcMaxP) void k_jc_terms(const double* __restrict__ state, const double* __restrict__ xy, int J,
                                                      const int* __restrict__ cand_count, const int* __restrict__ cand_lm,
                                                      int* __restrict__ head, int* __restrict__ offset,
                                                      int* __restrict__ reading_of, int* __restrict__ lm_of,
                                                      int* __restrict__ cols, double* __restrict__ Hc,
                                                      double* __restrict__ nu) {
    __shared__ int s_off[kJcMaxJ + 1];
    const int p = threadIdx.x, lane = p & 63;
    const double pv = state[lane < 3 ? lane : 0];   // as k_dlm_terms: three lanes load, every lane is still active
    const double theta = lane_bcast(pv, 0), x = lane_bcast(pv, 1), y = lane_bcast(pv, 2);
    if (p == 0) {
        int sum = 0;
        for (int j = 0; j < J; j++) {
            s_off[j] = sum;
            offset[j] = sum;
            const int n = cand_count[j];
            sum += n < 0 ? 0 : (n > kJcMaxC ? kJcMaxC : n);
        }
        s_off[J] = sum;
        head[0] = sum; head[1] = 0; head[2] = 0; head[3] = 0;
    }
    __syncthreads();
    if (p >= s_off[J]) return;
    int j = 0;
    while (j + 1 < J && s_off[j + 1] <= p) j++;   // (J is the bound; s_off is ascending and s_off [J] > p)
    const int i = cand_lm[j * kJcMaxC + (p - s_off[j])];
    reading_of[p] = j;
    lm_of[p] = i;
    const pair16 s = reinterpret_cast<const pair16*>(xy)[j];
    lm_store_terms(state, theta, x, y, s.x, s.y, i, p, 0, cols, Hc, nu);
}

// workgroup (bx, by): the blocks W[p][q] of p in [16 by, 16 by + 16), q in [16 bx, 16 bx + 16), P = head [0]
__global__ __launch_bounds__(kJcThreads) void k_jc_cross(const double* __restrict__ Sigma, int ld, const int* __restrict__ head,
                                                         const int* __restrict__ cols, const double* __restrict__ Hc,
                                                         double r_meas, int p_cap, double* __restrict__ W) {
    __shared__ double s_h[2][kJcTile][10], s_pose[3][3];
    __shared__ int s_c[2][kJcTile][2];
    int P = head[0];
    P = P < p_cap ? P : p_cap;   // (the buffer was cut for p_cap candidates)
    const int p0 = blockIdx.y * kJcTile, q0 = blockIdx.x * kJcTile, tid = threadIdx.x;
    if (p0 >= P || q0 >= P) return;   // (uniform over the workgroup)
    for (int e = tid; e < 2 * kJcTile * 10; e += kJcThreads) {
        const int side = e / (kJcTile * 10), r = e % (kJcTile * 10), c = (side ? q0 : p0) + r / 10;
        s_h[side][r / 10][r % 10] = c < P ? Hc[(size_t)c * 10 + r % 10] : 0.0;
    }
    for (int e = tid; e < 2 * kJcTile * 2; e += kJcThreads) {
        const int side = e / (kJcTile * 2), r = e % (kJcTile * 2), c = (side ? q0 : p0) + r / 2;
        s_c[side][r / 2][r % 2] = c < P ? cols[(size_t)c * 5 + 3 + r % 2] : 0;
    }
    if (tid < 9) s_pose[tid / 3][tid % 3] = Sigma[(size_t)(tid / 3) * ld + tid % 3];
    __syncthreads();
    const int tp = tid / kJcTile, tq = tid % kJcTile, p = p0 + tp, q = q0 + tq;
    if (p >= P || q >= P) return;
    int rp[5] = {0, 1, 2, s_c[0][tp][0], s_c[0][tp][1]}, cq[5] = {0, 1, 2, s_c[1][tq][0], s_c[1][tq][1]};
    double G[5][5];
#pragma unroll
    for (int k = 0; k < 5; k++)
#pragma unroll
        for (int b = 0; b < 5; b++) G[k][b] = (k < 3 && b < 3) ? s_pose[k][b] : Sigma[(size_t)rp[k] * ld + cq[b]];
    const double* hp = s_h[0][tp];
    const double* hq = s_h[1][tq];
    double T[2][5];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 5; b++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 5; k++) acc = fma(hp[a * 5 + k], G[k][b], acc);
            T[a][b] = acc;
        }
    double w[4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 5; k++) acc = fma(T[a][k], hq[b * 5 + k], acc);
            w[a * 2 + b] = p == q ? acc + (a == b ? r_meas : 0.0) : acc;
        }
    pair16* out = reinterpret_cast<pair16*>(W + ((size_t)p * P + q) * 4);
    out[0] = pair16{w[0], w[1]};
    out[1] = pair16{w[2], w[3]};
}

}  // namespace

void launch_dense64_jcbb_select(const double* nis, int n_readings, int count, int j0, int max_cand, double gate_ic,
                                double gate_new, int* cand_count, int* cand_lm, double* cand_nis, double* best, int* is_new,
                                hipStream_t st) {
    hipLaunchKernelGGL(k_jc_select, dim3(n_readings), dim3(kLmThreads), 0, st, nis, count, j0, max_cand, gate_ic, gate_new,
                       cand_count, cand_lm, cand_nis, best, is_new);
}

void launch_dense64_jcbb_terms(const double* state, const double* xy, int J, const int* cand_count, const int* cand_lm,
                               int* head, int* offset, int* reading_of, int* lm_of, int* cols, double* Hc, double* nu,
                               hipStream_t st) {
    hipLaunchKernelGGL(k_jc_terms, dim3(1), dim3(kJcMaxP), 0, st, state, xy, J, cand_count, cand_lm, head, offset, reading_of,
                       lm_of, cols, Hc, nu);
}

void launch_dense64_jcbb_cross(const double* Sigma, int ld, const int* head, const int* cols, const double* Hc, double r_meas,
                               int p_cap, double* W, hipStream_t st) {
    const int tiles = (p_cap + kJcTile - 1) / kJcTile;
    hipLaunchKernelGGL(k_jc_cross, dim3(tiles, tiles), dim3(kJcThreads), 0, st, Sigma, ld, head, cols, Hc, r_meas, p_cap, W);
}

}  // namespace ekf
