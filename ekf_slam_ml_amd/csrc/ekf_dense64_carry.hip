// ekf_dense64_carry.hip -- the pending rows of the dense fp64 handle (the deferred form of ekf_dense64_sparse.hip) CARRIED
// through the calls that used to flush them: the block-structured prediction, the (re)initialisation of a block and the
// block readout.
// The current covariance is Sigma_cur = Sigma_base - sum_{q < p} Kp[q]^T Tq[q].  propagate_block and init_block are
// congruences Sigma <- A Sigma A^T + Q with A the identity except in the r rows b = [first, first + r), and
//   A Sigma_cur A^T + Q = (A Sigma_base A^T + Q) - sum_q (A Kp[q]^T) (A Tq[q]^T)^T
// so k_d64_block / k_d64_init run on Sigma_base as they are and the pending rows take the map v <- A v, which changes the
// r entries v[b] of each row and nothing else.
//   k_dfp_map         v[first + a] <- sum_k M[a][k] v[src[k]] for the 2 p rows v of the two panels, one wave per row.
//                     propagate_block: M = Fr (r x r), src = b itself, in place; init_block: M = G (r x s), src = cols, and
//                     +0 when s = 0.  M^T sits in LDS as in k_d64_block (lane a reads Mt[k][a]: consecutive addresses); a
//                     wave loads the <= 64 source entries of its row in one instruction (lane k: v[src[k]]), parks them in
//                     LDS, and every lane a < r then walks them as broadcasts: all of a row's loads are issued before its
//                     first store.  2 p * r * s <= 128 * 64 * 64 multiply-adds in <= 32 workgroups: launch-bound.
//   k_dfp_read_block  k_d64_read_block (ekf_dense64_init.hip) plus the fold of ekf_dense64_sparse.hip: a workgroup owns
//                     256 consecutive entries of out, which touch <= 256 listed rows and <= 256 listed columns; their
//                     pending scalars Kp[q][rows[a]], Tq[q][cols[c]] go through LDS eight rows q at a time.
// The order (part of the contract, include/ekfslam.h).  Map: acc = +0; acc = fma(M[a][k], v[src[k]], acc) for k = 0, 1, ..
// -- exactly r (resp. s) terms, the same for both panels, a function of nothing but the block data.  Readout:
// x = Sigma_base[i][j]; x = fma(-Kp[q][i], Tq[q][j], x) for q = 0, 1, .. p - 1: the fold the deferred k_dsp_score applies
// to the block it reads.  fma() because the library is built with -ffp-contract=off.  No atomics.  Only columns
// [first, first + r) of rows q < p are written: the panels' padding (columns >= N) and their rows >= p are not touched.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

namespace {

constexpr int kMaxR = kDense64MaxR;
constexpr int kMaxS = kDense64MaxS;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;             // panel rows of a workgroup
constexpr int kBatch = kMaxR * kMaxS / kThreads;  // elements of M per thread

// Kp, Tq: the pending panels [64][ld], rows q < p mapped.  M: r x s row-major.  src: the s listed indices, or NULL for the
// block itself (then s == r).  Neither panel is __restrict__: both are read and written (disjoint rows per wave).
__global__ __launch_bounds__(kThreads) void k_dfp_map(double* Kp, double* Tq, int p, const double* __restrict__ M,
                                                      const int* __restrict__ src, int ld, int first, int r, int s) {
    extern __shared__ __attribute__((aligned(32))) double cm_smem[];
    const int r4 = (r + 3) & ~3;
    double* Mt = cm_smem;           // [s][r4]: Mt[k][a] = M[a][k]
    double* xs = Mt + s * r4;       // [kWaves][64]: the source entries of each wave's row
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int row = (int)blockIdx.x * kWaves + w;   // 0 .. p - 1: Kp, p .. 2 p - 1: Tq
    const bool live = row < 2 * p;                  // (uniform in the wave)
    double* v = live ? (row < p ? Kp + (size_t)row * ld : Tq + (size_t)(row - p) * ld) : nullptr;

    // Every global load is issued before the first of its results is used.
    double mv[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= s * r4) break;   // (uniform)
        const int e = t + b * kThreads;
        const int k = e / r4, a = e - k * r4;
        mv[b] = (e < s * r4 && a < r) ? M[a * s + k] : 0.0;
    }
    double x = 0.0;
    if (live && lane < s) x = v[src ? src[lane] : first + lane];
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= s * r4) break;
        const int e = t + b * kThreads;
        if (e < s * r4) Mt[e] = mv[b];
    }
    xs[w * 64 + lane] = x;
    __syncthreads();   // (every thread arrives: nothing returned above)
    if (!live || lane >= r) return;
    double acc = 0.0;
    for (int k = 0; k < s; k++) acc = fma(Mt[k * r4 + lane], xs[w * 64 + k], acc);
    v[first + lane] = acc;   // s == 0: +0
}

// out[a][c] = Sigma_cur[rows[a]][cols[c]]: the lanes along the column list
// LIVE (a live dimension below the handle's N, ekf_dense64_set_live): the pending rows have no support at indices >= live --
// what the panels hold there is left over from wider calls -- so an entry with such a row or column is returned as stored,
// and the panels are not read at those indices.  LIVE = false is the kernel as it was (`live` unused).
constexpr int kFoldRows = 8;
template <bool LIVE>
__global__ __launch_bounds__(kThreads) void k_dfp_read_block(const double* __restrict__ S, const double* __restrict__ Kp,
                                                             const double* __restrict__ Tq, int p,
                                                             const int* __restrict__ rows, const int* __restrict__ cols,
                                                             double* __restrict__ out, int nr, int nc, int ld, int live) {
    __shared__ double fk[kFoldRows][kThreads];   // Kp[q][rows[a0 + i]]
    __shared__ double ft[kFoldRows][kThreads];   // Tq[q][cols[..]]: index c when nc < 256, else the thread's own column
    const int t = threadIdx.x;
    const int total = nr * nc;
    const int e0 = (int)blockIdx.x * kThreads, e = e0 + t;
    const int e1 = min(e0 + kThreads, total) - 1;           // last entry of the workgroup
    const int a0 = e0 / nc, na = e1 / nc - a0 + 1;          // its listed rows: a0 .. a0 + na - 1, na <= 256
    const bool wide = nc >= kThreads;
    const int ncl = wide ? e1 - e0 + 1 : nc;                // its listed columns
    const bool real = e < total;
    const int a = real ? e / nc : 0, c = real ? e - a * nc : 0;
    const int my_row = t < na ? rows[a0 + t] : 0;                             // the row whose scalars this thread stages
    const int my_col = t < ncl ? cols[wide ? (e0 + t) % nc : t] : 0;          // the column likewise
    const int ia = a - a0, jc = wide ? t : c;
    double x = real ? S[(size_t)rows[a] * ld + cols[c]] : 0.0;
    bool folds = real;
    if constexpr (LIVE) folds = real && rows[a] < live && cols[c] < live;
    for (int q0 = 0; q0 < p; q0 += kFoldRows) {
        const int qs = min(kFoldRows, p - q0);
        double kv[kFoldRows], tv[kFoldRows];
#pragma unroll
        for (int q = 0; q < kFoldRows; q++) {   // every load of the chunk is issued before the first is used
            bool kin = q < qs && t < na, tin = q < qs && t < ncl;
            if constexpr (LIVE) kin = kin && my_row < live, tin = tin && my_col < live;
            kv[q] = kin ? Kp[(size_t)(q0 + q) * ld + my_row] : 0.0;
            tv[q] = tin ? Tq[(size_t)(q0 + q) * ld + my_col] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < kFoldRows; q++) fk[q][t] = kv[q], ft[q][t] = tv[q];
        __syncthreads();
        if (folds)
            for (int q = 0; q < qs; q++) x = fma(-fk[q][ia], ft[q][jc], x);
        __syncthreads();
    }
    if (real) out[e] = x;
}

size_t map_lds(int r, int s) { return sizeof(double) * ((size_t)s * ((r + 3) & ~3) + (size_t)kWaves * 64); }

}  // namespace

void launch_dense64_panel_map(double* Kp, double* Tq, int p, const double* M, const int* src, int ld, int first, int r,
                              int s, hipStream_t st) {
    if (p <= 0) return;
    hipLaunchKernelGGL(k_dfp_map, dim3((2 * p + kWaves - 1) / kWaves), dim3(kThreads), map_lds(r, s), st, Kp, Tq, p, M,
                       src, ld, first, r, s);
}

void launch_dense64_read_block_deferred(const double* Sigma, const double* Kp, const double* Tq, int p, const int* rows,
                                        const int* cols, double* out, int nr, int nc, int ld, int N, int live,
                                        hipStream_t st) {
    const dim3 grid((nr * nc + kThreads - 1) / kThreads);
    if (live < N)
        hipLaunchKernelGGL(k_dfp_read_block<true>, grid, dim3(kThreads), 0, st, Sigma, Kp, Tq, p, rows, cols, out, nr, nc, ld,
                           live);
    else
        hipLaunchKernelGGL(k_dfp_read_block<false>, grid, dim3(kThreads), 0, st, Sigma, Kp, Tq, p, rows, cols, out, nr, nc, ld,
                           live);
}

}  // namespace ekf
