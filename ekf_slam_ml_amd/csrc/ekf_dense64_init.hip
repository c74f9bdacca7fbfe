// ekf_dense64_init.hip -- landmark (re)initialisation on the dense fp64 covariance, and the small block readout.
// The states b = [first, first + r) are replaced by a new variable y = g(x[cols], z) with Jacobian G (r x s) with respect to
// the s listed states (none of them inside b) and W = Gz R Gz^T:
//   Sigma[b, j] <- G Sigma[cols, j]   (j outside b: s ROWS of Sigma)
//   Sigma[i, b] <- Sigma[i, cols] G^T (i outside b: s COLUMNS of Sigma; Sigma is never symmetrised)
//   Sigma[b, b] <- (G Sigma[cols, cols]) G^T + W                  state[b] <- xb
// which is F Sigma F^T + Q for F = identity with F[b, b] = 0, F[b, cols] = G and Q = zero with Q[b, b] = W.  s = 0 drops the
// block: its rows and columns become +0, its corner W, and Sigma is not read at all (the reference's constructor prior,
// rigid2d/src/ekf_slam.cpp:27-36, with W = 100 I; its initialize_landmark, :200-214, is the xb).
// ONE launch, three kinds of workgroup of one grid as in k_d64_block (ekf_dense64_block.hip):
//   block 0                 the corner and the state
//   blocks 1 .. n           row panel, a strip of 64 columns each: s row segments of 512 contiguous bytes in, r out
//   blocks n + 1 .. 2 n     column panel, a strip of 64 rows each: 64 segments of s gathered doubles in, of r contiguous
//                           doubles out
// Rows cols, columns cols and b are pairwise disjoint, so no input of any region is an output of any region: nothing is
// staged for the sake of an in-place update.  What is kept from k_d64_block / k_dsp_gather is about memory access: the
// column panel is loaded with the lanes running ALONG the list (neighbouring indices such as 0, 1, 2 share a cache line),
// transposed on the way into LDS (row stride 65 doubles: conflict-free both ways), and stored with the lanes along the r
// contiguous doubles of a segment; every global load of a phase is issued before its first use; G^T sits in LDS (a row of
// four consecutive a is one 32-byte broadcast read).  All three regions are one product out[a][c] = sum_k G[a][k] X[k][c]:
// for the corner X is the gathered block Sigma[cols, cols] and out is T' = G Sigma[cols, cols] (r x s), rounded to fp64,
// followed by S[a][d] = (sum_k T'[a][k] G[d][k]) + W[a][d].
// The order of every dot product: acc = +0; acc = fma(g_k, x_k, acc) for k = 0, 1, .. s - 1 of the list -- exactly s terms,
// one fused multiply-add per term (written as fma() because the library is built with -ffp-contract=off), a function of
// nothing but s.  W enters by one plain addition; without W there is no addition.  No atomics.  The corner is the order of
// k_dsp_score (ekf_dense64_sparse.hip) for S, so it is bit for bit the S of score_sparse(J = 1, m = r, s, cols, Hc = G,
// R = W) taken before the call; and the same source values give the same bits wherever they sit, in any N, on every run.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kMaxR = kDense64MaxR;
constexpr int kMaxS = kDense64MaxS;
constexpr int kStrip = 64;        // columns (rows) of a panel strip
constexpr int kXS = kStrip + 1;   // LDS row stride of X: conflict-free both ways
constexpr int kThreads = 256;
constexpr int kBatch = (kMaxR > kMaxS ? kMaxR : kMaxS) * kStrip / kThreads;   // elements of a tile per thread

__global__ __launch_bounds__(kThreads) void k_d64_init(double* __restrict__ S, double* __restrict__ state,
                                                       const int* __restrict__ cols, const double* __restrict__ G,
                                                       const double* __restrict__ W, const double* __restrict__ xb,
                                                       int N, int ld, int first, int r, int s, int n_strips) {
    extern __shared__ __attribute__((aligned(32))) double ini_smem[];
    const int r4 = (r + 3) & ~3;
    double* Gt = ini_smem;                  // [s][r4]: Gt[k][a] = G[a][k], zero for a >= r
    double* X = Gt + s * r4;                // [max(r, s)][kXS]: the inputs as X[k][c], later the results as X[a][c]
    int* lc = reinterpret_cast<int*>(X + max(r, s) * kXS);   // [s]
    const int t = threadIdx.x, c = t & 63, w = t >> 6;
    const int bid = blockIdx.x;
    const int kind = bid == 0 ? 2 : (bid <= n_strips ? 0 : 1);   // 0 row panel, 1 column panel, 2 corner
    const int base = kind == 2 ? 0 : (kind == 0 ? bid - 1 : bid - 1 - n_strips) * kStrip;   // first column / row
    const int last = first + r;
    if (kind != 2 && base >= first && min(base + kStrip, N) <= last) return;   // the strip lies inside the block (uniform)
    auto mine = [&](int cc) { const int p = base + cc; return p < N && (p < first || p >= last); };
    auto split = [&](int e, int n, int& k, int& cc) {   // lanes run along what is contiguous (or nearly so) in memory
        if (kind == 0) { k = e >> 6; cc = e & 63; }
        else if (kind == 1) { cc = e / n; k = e - cc * n; }
        else { k = e / n; cc = e - k * n; }
    };

    if (s == 0) {   // the block is dropped: +0 rows and columns, the corner is W; Sigma is not read
        if (kind == 2) {
            for (int e = t; e < r * r; e += kThreads) S[(size_t)(first + e / r) * ld + first + e % r] = W ? W[e] : 0.0;
            if (xb && t < r) state[first + t] = xb[t];
            return;
        }
        for (int e = t; e < r * kStrip; e += kThreads) {
            int k, cc;
            split(e, r, k, cc);
            if (mine(cc)) S[kind == 0 ? (size_t)(first + k) * ld + base + cc : (size_t)(base + cc) * ld + first + k] = 0.0;
        }
        return;
    }

    // Every global load of a phase is issued before the first of its results is used (at most kBatch = 16 per thread).
    double v[kBatch];
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= s * r4) break;   // (uniform)
        const int e = t + p * kThreads;
        const int k = e / r4, a = e - k * r4;
        v[p] = (e < s * r4 && a < r) ? G[a * s + k] : 0.0;
    }
    if (t < s) lc[t] = cols[t];
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= s * r4) break;
        const int e = t + p * kThreads;
        if (e < s * r4) Gt[e] = v[p];
    }
    __syncthreads();
    const int width = kind == 2 ? s : kStrip;   // columns of X in use
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= s * width) break;   // (uniform)
        const int e = t + p * kThreads;
        int k = 0, cc = 0;
        split(e, s, k, cc);
        double x = 0.0;
        if (e < s * width) {
            if (kind == 2) x = S[(size_t)lc[k] * ld + lc[cc]];
            else if (mine(cc)) x = kind == 0 ? S[(size_t)lc[k] * ld + base + cc] : S[(size_t)(base + cc) * ld + lc[k]];
        }
        v[p] = x;
    }
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= s * width) break;
        const int e = t + p * kThreads;
        int k = 0, cc = 0;
        split(e, s, k, cc);
        if (e < s * width) X[k * kXS + cc] = v[p];
    }
    __syncthreads();

    // out[a][c] = sum_k G[a][k] X[k][c], k ascending; wave w owns a = 16 q + 4 w + (0..3)
    double acc[4][4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int a0 = 16 * q + 4 * w;
#pragma unroll
        for (int u = 0; u < 4; u++) acc[q][u] = 0.0;
        if (a0 < r && c < width) {   // (a0: uniform in the wave)
            for (int k = 0; k < s; k++) {
                const double x = X[k * kXS + c];
                const f64x4 f = *reinterpret_cast<const f64x4*>(Gt + k * r4 + a0);
#pragma unroll
                for (int u = 0; u < 4; u++) acc[q][u] = fma(f[u], x, acc[q][u]);
            }
        }
    }
    if (kind == 0) {   // rows of Sigma: the lanes already run along 512 contiguous bytes
        if (mine(c)) {
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int a = 16 * q + 4 * w + u;
                    if (a < r) S[(size_t)(first + a) * ld + base + c] = acc[q][u];
                }
        }
        return;
    }
    __syncthreads();   // every wave has read X
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int a = 16 * q + 4 * w + u;
            if (a < r && c < width) X[a * kXS + c] = acc[q][u];
        }
    __syncthreads();
    if (kind == 1) {   // columns of Sigma: segments of r contiguous doubles, the lanes along them
#pragma unroll
        for (int p = 0; p < kBatch; p++) {
            if (p * kThreads >= r * kStrip) break;   // (uniform)
            const int e = t + p * kThreads;
            int k = 0, cc = 0;
            split(e, r, k, cc);
            if (e < r * kStrip && mine(cc)) S[(size_t)(base + cc) * ld + first + k] = X[k * kXS + cc];
        }
        return;
    }
    // the corner: X holds T'[a][k] = (G Sigma[cols, cols])[a][k], rounded; S[a][d] = (sum_k T'[a][k] G[d][k]) + W[a][d]
    for (int e = t; e < r * r; e += kThreads) {
        const int a = e / r, d = e - a * r;
        double sum = 0.0;
        for (int k = 0; k < s; k++) sum = fma(X[a * kXS + k], Gt[k * r4 + d], sum);
        if (W) sum = sum + W[e];
        S[(size_t)(first + a) * ld + first + d] = sum;
    }
    if (xb && t < r) state[first + t] = xb[t];
}

// out[a][c] = Sigma[rows[a]][cols[c]]: the lanes along the column list
__global__ __launch_bounds__(kThreads) void k_d64_read_block(const double* __restrict__ S, const int* __restrict__ rows,
                                                             const int* __restrict__ cols, double* __restrict__ out,
                                                             int nr, int nc, int ld) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= nr * nc) return;
    const int a = e / nc, c = e - a * nc;
    out[e] = S[(size_t)rows[a] * ld + cols[c]];
}

}  // namespace

size_t dense64_init_lds_bytes(int r, int s) {
    if (s == 0) return 0;
    return (sizeof(double) * ((size_t)s * ((r + 3) & ~3) + (size_t)(r > s ? r : s) * kXS) + sizeof(int) * (size_t)s + 15) &
           ~(size_t)15;
}

hipError_t dense64_init_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_d64_init), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)dense64_init_lds_bytes(kMaxR, kMaxS));
}

void launch_dense64_init(double* Sigma, double* state, const int* cols, const double* G, const double* W,
                         const double* xb, int N, int ld, int first, int r, int s, hipStream_t st) {
    const int n_strips = (N + kStrip - 1) / kStrip;
    hipLaunchKernelGGL(k_d64_init, dim3(1 + 2 * n_strips), dim3(kThreads), dense64_init_lds_bytes(r, s), st, Sigma, state,
                       cols, G, W, xb, N, ld, first, r, s, n_strips);
}

void launch_dense64_read_block(const double* Sigma, const int* rows, const int* cols, double* out, int nr, int nc, int ld,
                               hipStream_t st) {
    hipLaunchKernelGGL(k_d64_read_block, dim3((nr * nc + kThreads - 1) / kThreads), dim3(kThreads), 0, st, Sigma, rows,
                       cols, out, nr, nc, ld);
}

}  // namespace ekf
