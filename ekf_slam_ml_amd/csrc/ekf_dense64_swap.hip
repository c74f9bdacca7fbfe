// ekf_dense64_swap.hip -- the symmetric permutation that exchanges two blocks of states of the dense fp64 covariance:
// Sigma <- P Sigma P^T, state <- P state for the P that swaps A = [a, a + r) with B = [b, b + r), a + r <= b, and is the
// identity elsewhere.  What a map that REMOVES a landmark in its middle needs: swap it with the last live block, drop that
// (init_block, s = 0), shrink the live dimension.
//   Sigma[a + k][j] <-> Sigma[b + k][j]   for every column j outside A u B   (2 r ROWS)
//   Sigma[i][a + k] <-> Sigma[i][b + k]   for every row i outside A u B      (2 r COLUMNS; Sigma is never symmetrised)
//   Sigma[a + k][a + l] <-> Sigma[b + k][b + l],  Sigma[a + k][b + l] <-> Sigma[b + k][a + l]   (the 2 r x 2 r intersection:
//                                                                       the off-diagonal blocks are exchanged, not transposed)
//   state[a + k] <-> state[b + k]
// A pure copy: every entry keeps its bits (NaN payloads, -0.0).  ONE launch, three kinds of workgroup of one grid as in
// k_d64_init / k_d64_block:
//   block 0                 the intersection and the state: r * 2 r pairs, the lanes along the 2 r columns of a row of A
//   blocks 1 .. n           row panel, a strip of 64 columns each: r pairs of row segments, the lanes along 512 contiguous bytes
//   blocks n + 1 .. 2 n     column panel, a strip of 64 rows each: 64 pairs of segments of r contiguous doubles, the lanes
//                           along a segment
// A strip that lies wholly inside A u B returns at once (the intersection is block 0's); one that straddles a block boundary
// or N is masked element by element, so nothing at an index >= N is read or written -- N is the handle's LIVE dimension.
// Every entry has exactly one partner, and ONE thread owns the pair: it loads both and then stores both, crossed.  No entry
// is touched by two threads, let alone two workgroups, so there is nothing to stage and nothing to order: no LDS, no
// atomics, no barrier.  All global loads of a thread (at most 2 * 32 in block 0, 2 * 16 in a panel) are issued before its
// first store.
//   k_dfp_swap   the same exchange on the pending rows of the deferred corrections (ekf_dense64_carry.hip's algebra with
//                A = P): entries [a, a + r) and [b, b + r) of every row q < p of both panels, one wave per row, lane k owns
//                the pair (a + k, b + k).  The panels' padding and their rows >= p are not touched.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

namespace {

constexpr int kMaxR = kDense64MaxR;
constexpr int kStrip = 64;        // columns (rows) of a panel strip
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;                        // pending rows of a workgroup of k_dfp_swap
constexpr int kPanelBatch = kMaxR * kStrip / kThreads;       // pairs of a strip per thread: 16
constexpr int kCornerBatch = kMaxR * 2 * kMaxR / kThreads;   // pairs of the intersection per thread: 32

// The pairs [0, n) of one workgroup, kThreads at a time: where(e, ia, ib) gives the two offsets of pair e, or false for a
// pair that is masked.  Two passes over the same (uniform) trip count: every load, then every store.
template <int BATCH, class Where>
__device__ __forceinline__ void swap_pairs(double* S, int t, int n, Where where) {
    double u[BATCH], v[BATCH];
#pragma unroll
    for (int p = 0; p < BATCH; p++) {
        if (p * kThreads >= n) break;   // (uniform)
        size_t ia = 0, ib = 0;
        const int e = t + p * kThreads;
        const bool ok = e < n && where(e, ia, ib);
        u[p] = ok ? S[ia] : 0.0;
        v[p] = ok ? S[ib] : 0.0;
    }
#pragma unroll
    for (int p = 0; p < BATCH; p++) {
        if (p * kThreads >= n) break;
        size_t ia = 0, ib = 0;
        const int e = t + p * kThreads;
        if (e < n && where(e, ia, ib)) {
            S[ia] = v[p];
            S[ib] = u[p];
        }
    }
}

// a + r <= b (the launcher orders them).  S is read and written: not __restrict__.
__global__ __launch_bounds__(kThreads) void k_d64_swap(double* S, double* state, int N, int ld, int a, int b, int r,
                                                       int n_strips) {
    const int t = threadIdx.x;
    const int bid = blockIdx.x;
    if (bid == 0) {   // the intersection: pair e = (k, c) is row a + k at the c-th column of A u B and its image in row b + k
        double xa = 0.0, xb = 0.0;
        if (t < r) xa = state[a + t], xb = state[b + t];
        swap_pairs<kCornerBatch>(S, t, r * 2 * r, [&](int e, size_t& ia, size_t& ib) {
            const int k = e / (2 * r), c = e - k * 2 * r;
            ia = (size_t)(a + k) * ld + (c < r ? a + c : b + c - r);
            ib = (size_t)(b + k) * ld + (c < r ? b + c : a + c - r);
            return true;
        });
        if (t < r) state[a + t] = xb, state[b + t] = xa;
        return;
    }
    const int kind = bid <= n_strips ? 0 : 1;   // 0 row panel, 1 column panel
    const int base = (kind == 0 ? bid - 1 : bid - 1 - n_strips) * kStrip;   // first column / row of the strip
    const int end = min(base + kStrip, N);
    auto within = [&](int lo, int hi) { return base >= lo && end <= hi; };
    if (within(a, a + r) || within(b, b + r) || (b == a + r && within(a, b + r))) return;   // inside A u B (uniform)
    auto mine = [&](int cc) {
        const int p = base + cc;
        return p < N && (p < a || p >= a + r) && (p < b || p >= b + r);
    };
    if (kind == 0)   // rows a + k and b + k: the lanes run along 512 contiguous bytes
        swap_pairs<kPanelBatch>(S, t, r * kStrip, [&](int e, size_t& ia, size_t& ib) {
            const int k = e >> 6, cc = e & 63;
            ia = (size_t)(a + k) * ld + base + cc;
            ib = (size_t)(b + k) * ld + base + cc;
            return mine(cc);
        });
    else             // columns a + k and b + k: the lanes run along the r contiguous doubles of a segment
        swap_pairs<kPanelBatch>(S, t, r * kStrip, [&](int e, size_t& ia, size_t& ib) {
            const int cc = e / r, k = e - cc * r;
            ia = (size_t)(base + cc) * ld + a + k;
            ib = (size_t)(base + cc) * ld + b + k;
            return mine(cc);
        });
}

// Kp, Tq: the pending panels [64][ld]; rows q < p of both take v[a + k] <-> v[b + k].  One wave per row.
__global__ __launch_bounds__(kThreads) void k_dfp_swap(double* Kp, double* Tq, int p, int ld, int a, int b, int r) {
    const int lane = threadIdx.x & 63;
    const int row = (int)blockIdx.x * kWaves + (threadIdx.x >> 6);   // 0 .. p - 1: Kp, p .. 2 p - 1: Tq
    if (row >= 2 * p || lane >= r) return;
    double* v = row < p ? Kp + (size_t)row * ld : Tq + (size_t)(row - p) * ld;
    const double x = v[a + lane], y = v[b + lane];
    v[a + lane] = y;
    v[b + lane] = x;
}

}  // namespace

void launch_dense64_swap(double* Sigma, double* state, int N, int ld, int first_a, int first_b, int r, hipStream_t st) {
    const int n_strips = (N + kStrip - 1) / kStrip;
    const int a = first_a < first_b ? first_a : first_b, b = first_a < first_b ? first_b : first_a;
    hipLaunchKernelGGL(k_d64_swap, dim3(1 + 2 * n_strips), dim3(kThreads), 0, st, Sigma, state, N, ld, a, b, r, n_strips);
}

void launch_dense64_panel_swap(double* Kp, double* Tq, int p, int ld, int first_a, int first_b, int r, hipStream_t st) {
    if (p <= 0) return;
    hipLaunchKernelGGL(k_dfp_swap, dim3((2 * p + kWaves - 1) / kWaves), dim3(kThreads), 0, st, Kp, Tq, p, ld, first_a,
                       first_b, r);
}

}  // namespace ekf
