// ekf_dense64_block.hip -- block-structured prediction on the dense fp64 covariance: the reference's
//   sigma = At*sigma*At.t() + Q   (rigid2d/src/ekf_slam.cpp:101-102, association (At*sigma)*At.t() + Q)
// for At = identity with an r x r Jacobian Fr in the square b = [first, first + r) and Q zero outside it.  Only the block's
// rows and columns change:
//   Sigma[b, j] <- Fr Sigma[b, j]  (j outside b)     Sigma[i, b] <- Sigma[i, b] Fr^T  (i outside b)
//   Sigma[b, b] <- (Fr Sigma[b, b]) Fr^T + Qr        state[b] += dx
// ONE launch.  The three regions have disjoint inputs and outputs, so they are three kinds of workgroup of one grid:
//   block 0                 the corner (two passes, the longest job, so it starts first) and the state
//   blocks 1 .. n           row panel, a strip of 64 columns each: r x 64 doubles, every row 512 contiguous bytes
//   blocks n + 1 .. 2 n     column panel, a strip of 64 rows each: 64 segments of r doubles at stride ld
// Every workgroup brings its whole tile into LDS as X[k][c] (k = index inside the block, c = column resp. row of the
// strip) before it stores anything, so the update is in place.  The column panel is loaded with the lanes running ALONG a
// segment (element e of the strip = segment e / r, offset e % r): at r = 64 a wave reads one whole 512-byte segment, at
// small r consecutive lanes cover consecutive segments -- never a lane-private walk down one segment -- and the transpose
// happens on the way into LDS (row stride 65 doubles: conflict-free both ways).  Both panels are then the same product
//   out[a][c] = sum over k of Fr[a][k] * X[k][c]
// with Fr^T in LDS (a row of four consecutive a is one 32-byte broadcast read; measured against Fr in scalar registers,
// DESIGN.md 4.8.4).  A thread owns one c and up to sixteen a
// (wave w: a = 16 q + 4 w + 0..3), keeps them in registers until every wave has read X, writes them over X and the tile
// goes back the way it came.
// The order of every dot product: acc = +0; acc = fma(Fr[a][k], x[k], acc) for k = 0, 1, .. r - 1 -- exactly r terms, no
// padding in k, one fused multiply-add per term (v_fma_f64, written as fma() because the library is built with
// -ffp-contract=off), a function of nothing but r.  No atomics.  So the same block data gives the same bits at any
// `first`, in any N, on every run.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kMaxR = kDense64MaxR;
constexpr int kStrip = 64;        // columns (rows) of a panel strip
constexpr int kXS = kStrip + 1;   // LDS row stride of X
constexpr int kThreads = 256;
constexpr int kBatch = kMaxR * kStrip / kThreads;   // elements of a tile per thread

// acc[q][u] = sum_k Ft[k][16 q + 4 w + u] * X[k][c], k ascending
__device__ __forceinline__ void block_product(const double* __restrict__ Ft, const double* __restrict__ X, int r, int r4,
                                              int w, int c, double (&acc)[4][4]) {
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int a0 = 16 * q + 4 * w;
#pragma unroll
        for (int u = 0; u < 4; u++) acc[q][u] = 0.0;
        if (a0 < r) {   // (uniform in the wave)
            for (int k = 0; k < r; k++) {
                const double x = X[k * kXS + c];
                const f64x4 f = *reinterpret_cast<const f64x4*>(Ft + k * r4 + a0);
#pragma unroll
                for (int u = 0; u < 4; u++) acc[q][u] = fma(f[u], x, acc[q][u]);
            }
        }
    }
}

// X[a][c] = acc (transposed = false), or X[c][a] = acc for c < r (true: the corner, whose tile is r x r), for a < r
__device__ __forceinline__ void put_acc(double* __restrict__ X, int r, int w, int c, const double (&acc)[4][4],
                                        bool transposed) {
    if (transposed && c >= r) return;   // X has r rows
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int a = 16 * q + 4 * w + u;
            if (a < r) X[transposed ? c * kXS + a : a * kXS + c] = acc[q][u];
        }
}

__global__ __launch_bounds__(kThreads) void k_d64_block(double* __restrict__ S, double* __restrict__ state,
                                                        const double* __restrict__ Fr, const double* __restrict__ Qr,
                                                        const double* __restrict__ dx, int N, int ld, int first, int r,
                                                        int n_strips) {
    extern __shared__ __attribute__((aligned(32))) double blk_smem[];
    const int r4 = (r + 3) & ~3;
    double* Ft = blk_smem;        // [r][r4]: Ft[k][a] = Fr[a][k], zero for a >= r
    double* X = Ft + r * r4;      // [r][kXS]
    const int t = threadIdx.x, c = t & 63, w = t >> 6;
    const int bid = blockIdx.x;
    const int kind = bid == 0 ? 2 : (bid <= n_strips ? 0 : 1);   // 0 row panel, 1 column panel, 2 corner
    const int base = kind == 2 ? first : (kind == 0 ? bid - 1 : bid - 1 - n_strips) * kStrip;   // first column / row
    const int last = first + r;
    if (kind != 2 && base >= first && min(base + kStrip, N) <= last) return;   // the strip lies inside the block (uniform)

    // Every global load of a phase is issued before the first of its results is used (at most kBatch = 16 per thread:
    // r * 64 / 256), so a workgroup waits for memory once per phase and not once per element.
    double v[kBatch];
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= r * r4) break;   // (uniform: a small r stops after its first batch)
        const int e = t + p * kThreads;
        const int k = e / r4, a = e - k * r4;
        v[p] = (e < r * r4 && a < r) ? Fr[a * r + k] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= r * r4) break;
        const int e = t + p * kThreads;
        if (e < r * r4) Ft[e] = v[p];
    }
    // where element (k, cc) of the tile lives, or -1 when it is not this workgroup's to touch
    auto where = [&](int k, int cc) -> long long {
        const int p = base + cc;
        if (kind == 2) return cc < r ? (long long)(first + k) * ld + p : -1;
        if (p >= N || (p >= first && p < last)) return -1;
        return kind == 0 ? (long long)(first + k) * ld + p : (long long)p * ld + first + k;
    };
    auto split = [&](int e, int& k, int& cc) {   // lanes run along what is contiguous in memory
        if (kind == 1) { cc = e / r; k = e - cc * r; }
        else { k = e >> 6; cc = e & 63; }
    };
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= r * kStrip) break;
        const int e = t + p * kThreads;
        int k, cc;
        split(e, k, cc);
        const long long g = e < r * kStrip ? where(k, cc) : -1;
        v[p] = g >= 0 ? S[g] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= r * kStrip) break;
        const int e = t + p * kThreads;
        int k, cc;
        split(e, k, cc);
        if (e < r * kStrip) X[k * kXS + cc] = v[p];
    }
    __syncthreads();

    double acc[4][4];
    block_product(Ft, X, r, r4, w, c, acc);
    __syncthreads();   // every wave has read X
    if (kind == 2) {
        // T = Fr C sits in acc as T[a][c]; the second product out[d][a'] = sum_c Fr[d][c] T[a'][c] is the same routine on T^T
        put_acc(X, r, w, c, acc, true);
        __syncthreads();
        block_product(Ft, X, r, r4, w, c, acc);   // acc = out[d][a'] with d on the register axis, a' = this thread's c
        __syncthreads();
        put_acc(X, r, w, c, acc, true);           // X[a'][d]: rows of the corner again
        __syncthreads();
        for (int e = t; e < r * kStrip; e += kThreads) {
            const int k = e >> 6, cc = e & 63;
            if (cc < r) {
                double v = X[k * kXS + cc];
                if (Qr) v = v + Qr[k * r + cc];
                S[(long long)(first + k) * ld + first + cc] = v;
            }
        }
        if (dx && t < r) state[first + t] = state[first + t] + dx[t];
        return;
    }
    put_acc(X, r, w, c, acc, false);
    __syncthreads();
#pragma unroll
    for (int p = 0; p < kBatch; p++) {
        if (p * kThreads >= r * kStrip) break;
        const int e = t + p * kThreads;
        int k, cc;
        split(e, k, cc);
        const long long g = e < r * kStrip ? where(k, cc) : -1;
        if (g >= 0) S[g] = X[k * kXS + cc];
    }
}

}  // namespace

size_t dense64_block_lds_bytes(int r) { return sizeof(double) * ((size_t)r * ((r + 3) & ~3) + (size_t)r * kXS); }

hipError_t dense64_block_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_d64_block), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)dense64_block_lds_bytes(kMaxR));
}

void launch_dense64_block(double* Sigma, double* state, const double* Fr, const double* Qr, const double* dx, int N,
                          int ld, int first, int r, hipStream_t s) {
    const int n_strips = (N + kStrip - 1) / kStrip;
    hipLaunchKernelGGL(k_d64_block, dim3(1 + 2 * n_strips), dim3(kThreads), dense64_block_lds_bytes(r), s, Sigma, state,
                       Fr, Qr, dx, N, ld, first, r, n_strips);
}

}  // namespace ekf
