// ekf_dense64_invert.hpp -- the one device routine that inverts an m x m innovation covariance for the dense fp64 handle:
// Gauss-Jordan with partial pivoting on the augmented matrix [S | I] in LDS, then nu^T S^-1 nu.  Shared by the
// measurement update (k_dc_invert, ekf_dense64_correct.hip: one S, a workgroup) and the candidate scoring (k_ds_invert,
// ekf_dense64_score.hip: J of them, a workgroup or a wave each).  NT is the size of the thread group that works on one
// matrix: 256 (the workgroup, barriers are __syncthreads) or 64 (one wave, no workgroup barrier at all, so the waves of
// a workgroup are free to leave at different times).  Every element sees the same operations in the same order whatever
// NT is, so the two group sizes give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace ekf {

template <int NT>
__device__ __forceinline__ void gj_sync() {
    if constexpr (NT > 64) {
        __syncthreads();
    } else {   // one wave: DS operations of a wave complete in order; keep the compiler from moving them
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

template <int NT>
__device__ __forceinline__ int gj_any(int pred) {
    if constexpr (NT > 64) return __syncthreads_or(pred);
    else {
        gj_sync<NT>();
        return __any(pred);
    }
}

// What one matrix needs in LDS besides [S | I] itself.
struct GjScratch {
    double* prow;   // [2 m] the scaled pivot row
    double* fcol;   // [m]   the column being eliminated
    double* wv;     // [m]   S^-1 nu
    double* pv;     // [1]   the pivot
    int* ctl;       // [2]   pivot row, bad flag: written by the first wave before a barrier, read by everyone after it
};

// M: [m][stride] = [S | I] on entry (written by the group, not yet synchronised), [.. | S^-1] on a return of 0.
// t: this thread's index in the group, 0 .. NT - 1; every thread of the group calls.  Returns (uniformly over the group)
// 1 for a zero or non-finite pivot or an inverse that is not finite, 0 otherwise.  `bad_in`: this thread saw a non-finite
// entry of S while it filled M.
template <int NT>
__device__ __forceinline__ int gj_invert(double* M, int stride, const GjScratch& sc, int m, int t, int bad_in) {
    if (gj_any<NT>(bad_in)) return 1;   // a non-finite S
    for (int p = 0; p < m; p++) {
        if (t < 64) {   // the first wave: the row with the largest |entry| of column p at or below the diagonal (lowest index on a tie)
            const bool in = t >= p && t < m;
            const double x = in ? M[t * stride + p] : 0.0;
            double best = in ? fabs(x) : -1.0;
            int bi = t;
            const bool nonfinite = __any(in && !isfinite(x));
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const double ob = __shfl_xor(best, d);
                const int oi = __shfl_xor(bi, d);
                if (ob > best || (ob == best && oi < bi)) best = ob, bi = oi;
            }
            if (t == 0) {
                sc.ctl[0] = bi;
                sc.pv[0] = M[bi * stride + p];
                sc.ctl[1] = (nonfinite || !(best > 0.0)) ? 1 : 0;
            }
        }
        gj_sync<NT>();
        if (sc.ctl[1]) return 1;   // (uniform: read after the barrier, not written again) a zero or non-finite pivot
        const int pr = sc.ctl[0];
        const double pv = sc.pv[0];
        for (int c = t; c < 2 * m; c += NT) {   // swap rows p and pr, scale the pivot row
            const double x = M[pr * stride + c], y = M[p * stride + c];
            const double v = x / pv;
            M[pr * stride + c] = y;
            M[p * stride + c] = v;
            sc.prow[c] = v;
        }
        gj_sync<NT>();
        if (t < m) sc.fcol[t] = t == p ? 0.0 : M[t * stride + p];
        gj_sync<NT>();
        for (int e = t; e < m * 2 * m; e += NT) {
            const int r = e / (2 * m), c = e % (2 * m);
            if (r != p) M[r * stride + c] = M[r * stride + c] - sc.fcol[r] * sc.prow[c];
        }
        gj_sync<NT>();
    }
    int bad = 0;
    for (int e = t; e < m * m; e += NT)
        if (!isfinite(M[(e / m) * stride + m + e % m])) bad = 1;
    return gj_any<NT>(bad) ? 1 : 0;   // an inverse that overflowed
}

// nu^T S^-1 nu after gj_invert returned 0 (the score of calculate_maha_dis, ekf_slam.cpp:267-269): S^-1 nu row by row,
// then the dot product in ascending order.  The value is returned on thread 0 of the group (0.0 elsewhere).
template <int NT>
__device__ __forceinline__ double gj_quadratic(const double* M, int stride, const GjScratch& sc, int m, int t,
                                               const double* __restrict__ nu) {
    if (t < m) {
        double v = 0.0;
        for (int l = 0; l < m; l++) v += M[t * stride + m + l] * nu[l];
        sc.wv[t] = v;
    }
    gj_sync<NT>();
    double v = 0.0;
    if (t == 0)
        for (int k = 0; k < m; k++) v += nu[k] * sc.wv[k];
    return v;
}

}  // namespace ekf
