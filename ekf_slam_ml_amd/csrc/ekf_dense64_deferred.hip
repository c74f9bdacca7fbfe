// ekf_dense64_deferred.hip -- the column-sparse correction and scoring of the dense fp64 handle READ THROUGH corrections
// that have not been applied to Sigma yet.  The handle keeps p <= 64 pending rows of two panels [64][ld],
//   Kp[q][i] = K[i][q]  (the gain of k_dc_gain, ekf_dense64_correct.hip)      Tq[q][j] = T[q][j] = (H Sigma_cur)[q][j]
// and the covariance every call sees is   Sigma_cur[i][j] = Sigma[i][j] - sum_{q < p} Kp[q][i] Tq[q][j]
// with Sigma in memory left alone until the flush (ONE launch of k_dc_update at rank p instead of one per correction).
//   k_dfp_gather   the twin of k_dsp_gather (ekf_dense64_sparse.hip): the same grid, lane maps and transposes through
//                  LDS; between the gather of X and the product the pending rows are folded into X.  A row strip
//                  (X[k][c] = Sigma[cols[k]][base + c]) reads Tq[q][strip] contiguously and the p * s scalars
//                  Kp[q][cols[k]] from LDS; a column strip (X[k][c] = Sigma[base + c][cols[k]]) reads Kp[q][strip]
//                  contiguously and the scalars Tq[q][cols[k]].  T is written into rows p .. p + m - 1 of the pending T
//                  panel (the rows read, q < p, and the rows written are disjoint), U^T where k_dc_gain reads it.
//   k_dfp_score    the twin of k_dsp_score in its wave and its workgroup form: the gathered s x s block G is folded the
//                  same way before T' = Hc G, the pending scalars Kp[q][cols[a]], Tq[q][cols[b]] going through LDS sixteen
//                  rows q at a time; everything after that is k_dsp_score's code.  The deferred correction launches it
//                  with J = 1 (S^-1 written out), so a score and the deferred correction that follows it with the same
//                  operands see the same S, nis and verdict bit for bit, with rows pending too.
// The order of the fold (part of the contract, include/ekfslam.h): x = fma(-Kp[q][row], Tq[q][col], x) for q = 0, 1, ..
// p - 1, one fused multiply-add per pending row (fma() because the library is built with -ffp-contract=off), before the
// first term of any dot product; the dot products are those of ekf_dense64_sparse.hip.  No atomics.  With p = 0 nothing is
// folded and both kernels do the arithmetic of their twins on the same operands.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense64_invert.hpp"

namespace ekf {

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kMaxM = kDense64MaxM;
constexpr int kMaxS = kDense64MaxS;
constexpr int kMaxP = kDense64PendingMaxRows;
constexpr int kStrip = 64;        // columns (rows) of a panel strip
constexpr int kXS = kStrip + 1;   // LDS row stride of X: conflict-free both ways
constexpr int kThreads = 256;
constexpr int kBatch = kMaxS * kStrip / kThreads;   // elements of a tile per thread
static_assert(kMaxP * kStrip <= kBatch * kThreads && kMaxP * kMaxS <= kBatch * kThreads, "a batch holds the pending rows");

// ---- the panels ----------------------------------------------------------------------------------------------------------
// Kp, Tq: the pending panels [64][ld], rows q < p read; Tout = Tq + p * ld and Ut: [m][ld], written up to ld.
// (Tq and Tout are one buffer: neither is __restrict__.)
__global__ __launch_bounds__(kThreads) void k_dfp_gather(const double* __restrict__ S, const int* __restrict__ cols,
                                                         const double* __restrict__ Hc, const double* Kp, const double* Tq,
                                                         double* Tout, double* __restrict__ Ut, int N, int ld, int m,
                                                         int s, int p, int n_strips) {
    extern __shared__ __attribute__((aligned(32))) double df_smem[];
    const int m4 = (m + 3) & ~3;
    double* Hct = df_smem;            // [s][m4]: Hct[k][a] = Hc[a][k], zero for a >= m
    double* X = Hct + s * m4;         // [s][kXS]
    double* strip = X + s * kXS;      // [p][kStrip]: the pending panel that runs along the strip
    double* scal = strip + p * kStrip;   // [p][s]: the other panel at the listed indices
    int* lc = reinterpret_cast<int*>(scal + p * s);   // [s]
    const int t = threadIdx.x, c = t & 63, w = t >> 6;
    const int kind = (int)blockIdx.x >= n_strips ? 1 : 0;   // 0: columns of T, 1: rows of U^T
    const int base = ((int)blockIdx.x - kind * n_strips) * kStrip;

    // Every global load of a phase is issued before the first of its results is used (at most kBatch = 16 per array).
    double v[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= s * m4) break;   // (uniform)
        const int e = t + b * kThreads;
        const int k = e / m4, a = e - k * m4;
        v[b] = (e < s * m4 && a < m) ? Hc[a * s + k] : 0.0;
    }
    if (t < s) lc[t] = cols[t];
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= s * m4) break;
        const int e = t + b * kThreads;
        if (e < s * m4) Hct[e] = v[b];
    }
    __syncthreads();
    auto split = [&](int e, int& k, int& cc) {   // lanes run along what is contiguous (or nearly so) in memory
        if (kind == 1) { cc = e / s; k = e - cc * s; }
        else { k = e >> 6; cc = e & 63; }
    };
    const double* along = kind == 0 ? Tq : Kp;    // read at [q][base + cc]
    const double* listed = kind == 0 ? Kp : Tq;   // read at [q][cols[k]]
    double sv[kBatch], cv[kBatch];
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= s * kStrip) break;
        const int e = t + b * kThreads;
        int k = 0, cc = 0;
        split(e, k, cc);
        double x = 0.0;
        if (e < s * kStrip && base + cc < N)
            x = kind == 0 ? S[(size_t)lc[k] * ld + base + cc] : S[(size_t)(base + cc) * ld + lc[k]];
        v[b] = x;
    }
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= p * kStrip) break;
        const int e = t + b * kThreads;
        const int q = e >> 6, cc = e & 63;
        sv[b] = (q < p && base + cc < N) ? along[(size_t)q * ld + base + cc] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= p * s) break;
        const int e = t + b * kThreads;
        const int q = e / s, k = e - q * s;
        cv[b] = q < p ? listed[(size_t)q * ld + lc[k]] : 0.0;
    }
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= s * kStrip) break;
        const int e = t + b * kThreads;
        int k = 0, cc = 0;
        split(e, k, cc);
        if (e < s * kStrip) X[k * kXS + cc] = v[b];
    }
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= p * kStrip) break;
        const int e = t + b * kThreads;
        if (e < p * kStrip) strip[e] = sv[b];
    }
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= p * s) break;
        const int e = t + b * kThreads;
        if (e < p * s) scal[e] = cv[b];
    }
    __syncthreads();

    // X[k][c] -= sum_q Kp[q][row] Tq[q][col], q ascending; wave w owns k = w, w + 4, ..
    if (p > 0) {   // (uniform)
        double xr[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; b++) {
            const int k = w + 4 * b;
            if (4 * b >= s) break;
            xr[b] = k < s ? X[k * kXS + c] : 0.0;
        }
        for (int q = 0; q < p; q++) {
            const double along_q = strip[q * kStrip + c];
#pragma unroll
            for (int b = 0; b < kBatch; b++) {
                const int k = w + 4 * b;
                if (4 * b >= s) break;
                if (k < s) xr[b] = fma(-scal[q * s + k], along_q, xr[b]);   // (the product is the same either way round)
            }
        }
#pragma unroll
        for (int b = 0; b < kBatch; b++) {
            const int k = w + 4 * b;
            if (4 * b >= s) break;
            if (k < s) X[k * kXS + c] = xr[b];
        }
        __syncthreads();
    }

    // out[a][c] = sum_k Hc[a][k] X[k][c], k ascending; wave w owns a = 16 q + 4 w + (0..3)
    double* out = (kind == 0 ? Tout : Ut) + base + c;
    const bool real = base + c < N;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int a0 = 16 * q + 4 * w;
        if (a0 >= m) break;   // (uniform in the wave)
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < s; k++) {
            const double x = X[k * kXS + c];
            const f64x4 f = *reinterpret_cast<const f64x4*>(Hct + k * m4 + a0);
#pragma unroll
            for (int u = 0; u < 4; u++) acc[u] = fma(f[u], x, acc[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
            if (a0 + u < m) out[(size_t)(a0 + u) * ld] = real ? acc[u] : 0.0;   // the panels' padding is zero
    }
}

// ---- S, its inverse, flag, nis of one candidate --------------------------------------------------------------------------
// LDS of a candidate, in doubles: the layout of k_dsp_score (Hc [m][s] | G [s][s], T' [m][s] -- later [S | I] over both |
// 4 m + 1 of scratch) | fk [16][s], ft [16][s]: the pending scalars of sixteen rows q.  The index lists and the control
// words of all candidates of the workgroup follow as ints.
constexpr int kFoldRows = 16;
__host__ __device__ constexpr int score_big(int m, int s) {
    return s * s + m * s > m * (2 * m + 1) ? s * s + m * s : m * (2 * m + 1);
}
__host__ __device__ constexpr int score_base_doubles(int m, int s) {
    return (m * s + score_big(m, s) + 4 * m + 1 + 1) & ~1;
}
__host__ __device__ constexpr int score_cand_doubles(int m, int s) {
    return score_base_doubles(m, s) + 2 * kFoldRows * s;
}
constexpr size_t score_lds(int per, int m, int s) {
    return ((sizeof(double) * (size_t)per * score_cand_doubles(m, s) + sizeof(int) * (size_t)per * (s + 2)) + 15) &
           ~(size_t)15;
}
constexpr int kWaveM = 16;                   // up to here a wave per candidate, LDS permitting
constexpr size_t kWaveLds = 64 * 1024;       // what four candidates of a workgroup may take together

// The arguments of k_dsp_score plus the pending panels Kp, Tq [64][ld] and their row count p.
template <int NT, int EPT>
__global__ __launch_bounds__(kThreads) void k_dfp_score(const double* __restrict__ Sigma, const double* __restrict__ Kp,
                                                        const double* __restrict__ Tq, int p,
                                                        const int* __restrict__ cols, const double* __restrict__ Hc,
                                                        const double* __restrict__ R, int r_shared,
                                                        const double* __restrict__ nu, double* __restrict__ nis,
                                                        double* __restrict__ S_out, int* __restrict__ flag,
                                                        double* __restrict__ Sinv, int ld, int m, int s, int J) {
    extern __shared__ __attribute__((aligned(32))) double df_smem[];
    constexpr int PER = kThreads / NT;
    constexpr int FB = kFoldRows * kMaxS / NT;   // pending scalars of a chunk per thread and panel
    const int sub = threadIdx.x / NT, t = threadIdx.x % NT;
    const int cand = blockIdx.x * PER + sub;
    if (cand >= J) return;   // (uniform over the candidate's thread group; NT = 64 takes no workgroup barrier)
    const int cd = score_cand_doubles(m, s), mm = m * m, ms = m * s, stride = 2 * m + 1;
    double* hc = df_smem + sub * cd;     // [m][s]
    double* G = hc + ms;                 // [s][s] = Sigma_cur[cols, cols]
    double* Tl = G + s * s;              // [m][s] = Hc G
    double* M = G;                       // [m][stride], once G and T' are spent
    double* tail = G + score_big(m, s);
    double* fk = hc + score_base_doubles(m, s);   // [kFoldRows][s]: Kp[q][cols[a]]
    double* ft = fk + kFoldRows * s;              // [kFoldRows][s]: Tq[q][cols[b]]
    int* lc = reinterpret_cast<int*>(df_smem + PER * cd) + sub * (s + 2);
    const GjScratch sc{tail, tail + 2 * m, tail + 3 * m, tail + 4 * m, lc + s};

    for (int e = t; e < s; e += NT) lc[e] = cols[(size_t)cand * s + e];
    for (int e = t; e < ms; e += NT) hc[e] = Hc[(size_t)cand * ms + e];
    gj_sync<NT>();
    for (int e = t; e < s * s; e += NT) {   // lanes along the list: neighbouring indices share a cache line
        const int a = e / s, b = e - a * s;
        G[e] = Sigma[(size_t)lc[a] * ld + lc[b]];
    }
    gj_sync<NT>();
    for (int q0 = 0; q0 < p; q0 += kFoldRows) {   // G[a][b] -= sum_q Kp[q][cols[a]] Tq[q][cols[b]], q ascending
        const int qs = min(kFoldRows, p - q0) * s;
        double kv[FB], tv[FB];
#pragma unroll
        for (int i = 0; i < FB; i++) {   // every load of the chunk is issued before the first is used
            if (i * NT >= qs) break;     // (uniform)
            const int e = t + i * NT;
            kv[i] = 0.0, tv[i] = 0.0;
            if (e < qs) {
                const size_t off = (size_t)(q0 + e / s) * ld + lc[e % s];
                kv[i] = Kp[off];
                tv[i] = Tq[off];
            }
        }
#pragma unroll
        for (int i = 0; i < FB; i++) {
            if (i * NT >= qs) break;
            const int e = t + i * NT;
            if (e < qs) fk[e] = kv[i], ft[e] = tv[i];
        }
        gj_sync<NT>();
        for (int e = t; e < s * s; e += NT) {   // (the elements this thread gathered)
            const int a = e / s, b = e - a * s;
            double g = G[e];
            for (int q = 0; q * s < qs; q++) g = fma(-fk[q * s + a], ft[q * s + b], g);
            G[e] = g;
        }
        gj_sync<NT>();
    }
    for (int e = t; e < ms; e += NT) {      // T'[a][b] = T[a][cols[b]] = sum_k Hc[a][k] Sigma_cur[cols[k]][cols[b]]
        const int a = e / s, b = e - a * s;
        double acc = 0.0;
        for (int k = 0; k < s; k++) acc = fma(hc[a * s + k], G[k * s + b], acc);
        Tl[e] = acc;
    }
    gj_sync<NT>();
    const double* Rc = R + (r_shared ? 0 : (size_t)cand * mm);
    double sv[EPT];
    int bad = 0;
#pragma unroll
    for (int q = 0; q < EPT; q++) {
        const int e = t + NT * q;
        sv[q] = 0.0;
        if (e < mm) {
            const int a = e / m, b = e - a * m;
            double acc = 0.0;
            for (int k = 0; k < s; k++) acc = fma(Tl[a * s + k], hc[b * s + k], acc);
            const double val = acc + Rc[e];
            if (!isfinite(val)) bad = 1;
            if (S_out) S_out[(size_t)cand * mm + e] = val;
            sv[q] = val;
        }
    }
    gj_sync<NT>();   // every thread of the group is done with G and T'
#pragma unroll
    for (int q = 0; q < EPT; q++) {
        const int e = t + NT * q;
        if (e < mm) {
            const int a = e / m, b = e - a * m;
            M[a * stride + b] = sv[q];
            M[a * stride + m + b] = a == b ? 1.0 : 0.0;
        }
    }
    const int verdict = gj_invert<NT>(M, stride, sc, m, t, bad);   // (uniform over the group)
    if (Sinv && cand == 0 && !verdict)
        for (int e = t; e < mm; e += NT) Sinv[(e / m) * kMaxM + e % m] = M[(e / m) * stride + m + e % m];
    double val = __builtin_nan("");
    if (nis && !verdict) val = gj_quadratic<NT>(M, stride, sc, m, t, nu + (size_t)cand * m);
    if (t == 0) {
        if (nis) nis[cand] = val;
        flag[cand] = verdict;
    }
}

size_t gather_lds(int m, int s, int p) {
    return (sizeof(double) * ((size_t)s * ((m + 3) & ~3) + (size_t)s * kXS + (size_t)p * kStrip + (size_t)p * s) +
            sizeof(int) * (size_t)s + 15) & ~(size_t)15;
}

}  // namespace

hipError_t dense64_deferred_prepare() {
    // gather: 128.8 KiB at m = s = p = 64; scoring: 64 KiB for four waves, 114.8 KiB for the workgroup at m = s = 64
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_dfp_gather),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)gather_lds(kMaxM, kMaxS, kMaxP));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dfp_score<64, 4>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWaveLds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dfp_score<256, 16>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)score_lds(1, kMaxM, kMaxS));
}

void launch_dense64_score_deferred(const double* Sigma, const double* Kp, const double* Tq, int p, const int* cols,
                                   const double* Hc, const double* R, int r_shared, const double* nu, int J, int m, int s,
                                   int ld, double* nis, double* S_out, int* flag, double* Sinv, hipStream_t st) {
    if (m <= kWaveM && score_lds(4, m, s) <= kWaveLds)
        hipLaunchKernelGGL((k_dfp_score<64, 4>), dim3((J + 3) / 4), dim3(kThreads), score_lds(4, m, s), st, Sigma, Kp, Tq,
                           p, cols, Hc, R, r_shared, nu, nis, S_out, flag, Sinv, ld, m, s, J);
    else
        hipLaunchKernelGGL((k_dfp_score<256, 16>), dim3(J), dim3(kThreads), score_lds(1, m, s), st, Sigma, Kp, Tq, p,
                           cols, Hc, R, r_shared, nu, nis, S_out, flag, Sinv, ld, m, s, J);
}

void launch_dense64_correct_deferred(const Dense64CorrectPlan& pl, const double* Sigma, double* state, double* ws,
                                     double* Kp, double* Tq, int p, const int* cols, const double* Hc, const double* R,
                                     const double* nu, int m, int s, double* nis, int* verdict, hipStream_t st) {
    const int n_strips = pl.ld / kStrip;   // ld is a multiple of 128: the panels are written up to ld
    hipLaunchKernelGGL(k_dfp_gather, dim3(2 * n_strips), dim3(kThreads), gather_lds(m, s, p), st, Sigma, cols, Hc, Kp, Tq,
                       Tq + (size_t)p * pl.ld, ws + pl.off_Ut, pl.N, pl.ld, m, s, p, n_strips);
    launch_dense64_score_deferred(Sigma, Kp, Tq, p, cols, Hc, R, 1, nu, 1, m, s, pl.ld, nu ? nis : nullptr, nullptr,
                                  verdict, ws + pl.off_Sinv, st);
    launch_dense64_gain(pl, ws, Kp + (size_t)p * pl.ld, state, nu, m, verdict, st);
}

}  // namespace ekf
