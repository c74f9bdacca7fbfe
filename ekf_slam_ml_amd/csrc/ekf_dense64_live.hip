// ekf_dense64_live.hip -- the check that goes with the live dimension of the dense fp64 handle (ekf_dense64_set_live): with
// live = Na < N the structured calls run the filter of dimension Na in Sigma[0:Na, 0:Na], which equals the full-width call
// exactly when the tail is DECOUPLED, Sigma[i][j] = 0 whenever exactly one of i, j is >= Na.  k_d64_coupling measures that:
// over the two off-diagonal rectangles
//   rows [0, Na)  x columns [Na, N)     Na segments of N - Na contiguous doubles
//   rows [Na, N)  x columns [0, Na)     N - Na segments of Na contiguous doubles (the rectangle under the diagonal, read as
//                                       rows as well: Sigma is never assumed symmetric)
// it counts the entries != 0 (-0.0 is zero; a NaN counts) and takes the largest |entry|.  16 Na (N - Na) bytes are read
// once, nothing of Sigma is written.  A workgroup takes rows blockIdx.x, + gridDim.x, ..; its lanes run along the row's
// segment, four independent loads in flight per thread; the partial results go wave -> workgroup through shuffles and
// LDS and then into two 64-bit words by INTEGER atomics (an addition and a maximum of the bit patterns of |x|, which order
// as the values do for everything that is not a NaN and put every NaN above infinity).  Integer addition and maximum are
// associative, so the outputs are the same bits on every run whatever the order the workgroups arrive in.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;
constexpr int kMaxGroups = 2048;   // eight workgroups per CU: enough loads in flight to stream, few enough atomics

__global__ __launch_bounds__(kThreads) void k_d64_coupling(const double* __restrict__ S, int N, int ld, int Na,
                                                           unsigned long long* __restrict__ out) {
    __shared__ unsigned long long wc[kThreads / 64], wm[kThreads / 64];
    const int t = threadIdx.x;
    unsigned long long count = 0, most = 0;
    auto take = [&](double x) {
        if (x != 0.0) count++;   // (NaN != 0 holds)
        const unsigned long long bits = (unsigned long long)__double_as_longlong(x) & 0x7fffffffffffffffull;
        most = bits > most ? bits : most;
    };
    for (int row = blockIdx.x; row < N; row += gridDim.x) {
        const int c0 = row < Na ? Na : 0, c1 = row < Na ? N : Na;   // the row's segment [c0, c1)
        const double* p = S + (size_t)row * ld;
        int c = c0 + t;
        for (; c + (kUnroll - 1) * kThreads < c1; c += kUnroll * kThreads) {
            double x[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) x[u] = p[c + u * kThreads];
#pragma unroll
            for (int u = 0; u < kUnroll; u++) take(x[u]);
        }
        for (; c < c1; c += kThreads) take(p[c]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        count += __shfl_down(count, off);
        const unsigned long long o = __shfl_down(most, off);
        most = o > most ? o : most;
    }
    if ((t & 63) == 0) wc[t >> 6] = count, wm[t >> 6] = most;
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kThreads / 64; w++) {
            count += wc[w];
            most = wm[w] > most ? wm[w] : most;
        }
        if (count) atomicAdd(out, count);
        if (most) atomicMax(out + 1, most);
    }
}

}  // namespace

void launch_dense64_coupling(const double* Sigma, int N, int ld, int Na, unsigned long long* out, hipStream_t st) {
    if (Na >= N) return;   // no rectangle: the zeroed words stand
    hipLaunchKernelGGL(k_d64_coupling, dim3(N < kMaxGroups ? N : kMaxGroups), dim3(kThreads), 0, st, Sigma, N, ld, Na, out);
}

}  // namespace ekf
