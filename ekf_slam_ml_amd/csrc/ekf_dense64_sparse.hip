// ekf_dense64_sparse.hip -- the measurement update and the candidate scoring of the dense fp64 handle for a Jacobian that
// is zero outside s listed columns (1 <= s <= 64): H[:, cols[k]] = Hc[:, k].  The reference's Hj has five such columns
// (rigid2d/src/ekf_slam.cpp:140-178: the pose columns 0, 1, 2 and the landmark columns 3 + 2 i, 4 + 2 i), so
//   T = H Sigma  is a combination of s ROWS of Sigma,     T[a][j] = sum_k Hc[a][k] Sigma[cols[k]][j]
//   U = Sigma H^T  of s COLUMNS (Sigma is never symmetrised), U[i][a] = sum_k Sigma[i][cols[k]] Hc[a][k]
//   S = T H^T + R  needs the s x s block Sigma[cols, cols] only, S[a][b] = (sum_k T[a][cols[k]] Hc[b][k]) + R[a][b]
// and neither call has to stream Sigma to build them.  Both kernels are compiled twice from one source: the EAGER form
// (Eager) reads Sigma as it sits in memory; the DEFERRED form (Pending) READS THROUGH corrections that have not been
// applied to Sigma yet.  For those the handle keeps p <= 64 pending rows of two panels [64][ld],
//   Kp[q][i] = K[i][q]  (the gain of k_dc_gain, ekf_dense64_correct.hip)      Tq[q][j] = T[q][j] = (H Sigma_cur)[q][j]
// and the covariance every call sees is   Sigma_cur[i][j] = Sigma[i][j] - sum_{q < p} Kp[q][i] Tq[q][j]
// with Sigma in memory left alone until the flush (ONE launch of k_dc_update at rank p instead of one per correction).
// The switch is a compile-time one because the eager form is the lean one: 64 against 106 VGPRs in the gather, 58 against
// 136 in the wave form of the scoring, half the LDS.
//   k_dsp_gather   the two panels of a correction: workgroups 0 .. n - 1 a strip of 64 columns of T each (s row segments of
//                  512 contiguous bytes), workgroups n .. 2 n - 1 a strip of 64 rows of U^T each (64 segments of s gathered
//                  doubles, loaded with the lanes running ALONG the list so that neighbouring indices such as 0, 1, 2 share
//                  a cache line; the transpose happens on the way through LDS, as in k_d64_block).  Both are then one
//                  product out[a][c] = sum_k Hc[a][k] X[k][c] with Hc^T in LDS; the panels' padding (c >= N) is written as
//                  zero.  Eager: T and U^T go where k_dc_gain / k_dc_update (ekf_dense64_correct.hip) read them.  Deferred:
//                  between the gather of X and the product the pending rows are folded into X.  A row strip
//                  (X[k][c] = Sigma[cols[k]][base + c]) reads Tq[q][strip] contiguously and the p * s scalars
//                  Kp[q][cols[k]] from LDS; a column strip (X[k][c] = Sigma[base + c][cols[k]]) reads Kp[q][strip]
//                  contiguously and the scalars Tq[q][cols[k]].  T is written into rows p .. p + m - 1 of the pending T
//                  panel (the rows read, q < p, and the rows written are disjoint), U^T where k_dc_gain reads it.
//   k_dsp_score    per candidate: cols and Hc into LDS, the s x s block G gathered, T' = Hc G (m x s, rounded to fp64), S,
//                  the elimination of ekf_dense64_invert.hpp, flag, nis.  A wave per candidate (four to a workgroup)
//                  where m <= 16 and four candidates fit 64 KiB of LDS, a workgroup per candidate otherwise; the same
//                  operations in the same order either way.  Deferred: G is folded as X is before T' = Hc G, the pending
//                  scalars Kp[q][cols[a]], Tq[q][cols[b]] going through LDS sixteen rows q at a time; everything after
//                  that is the same code.  ekf_dense64_score_sparse is ONE launch of it over J candidates; both forms of
//                  the correction launch it with J = 1 (and S^-1 written out), so a score and the correction that follows
//                  it with the same operands see the same S, nis and verdict bit for bit, with rows pending too.
// The order of every dot product: acc = +0; acc = fma(x_k, y_k, acc) for k = 0, 1, .. s - 1 of the list -- exactly s
// terms, one fused multiply-add per term (written as fma() because the library is built with -ffp-contract=off), a
// function of nothing but s.  R enters by one plain addition.  No atomics.  So the same Sigma[cols, cols], Hc, R, nu give
// the same bits wherever the columns sit, in any N, at any position of any batch, on every run.
// The order of the fold (part of the contract, include/ekfslam.h): x = fma(-Kp[q][row], Tq[q][col], x) for q = 0, 1, ..
// p - 1, one fused multiply-add per pending row, before the first term of any dot product.  With p = 0 nothing is folded
// and the deferred form does the arithmetic of the eager one on the same operands.
#include <hip/hip_runtime.h>

#include <type_traits>

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

// What a kernel reads Sigma through: nothing, or rows q < p of the pending panels Kp, Tq [64][ld].  Tout: how the gather
// takes the panel it writes T to -- the deferred form writes rows of the buffer it reads Tq from, so not __restrict__ there.
struct Eager {
    static constexpr int p = 0;
    using Tout = double* __restrict__;
};
struct Pending {
    const double* Kp;
    const double* Tq;
    int p;
    using Tout = double*;
};
template <class PEND>
constexpr bool kFolds = std::is_same<PEND, Pending>::value;

// ---- the panels --------------------------------------------------------------------------------------------------------
// Tout, Ut: [m][ld] (row stride ld), written up to ld.  Eager: the layout of Dense64CorrectPlan::off_T / off_Ut.  Deferred:
// Tout = Tq + p * ld.
template <class PEND>
__global__ __launch_bounds__(kThreads) void k_dsp_gather(const double* __restrict__ S, const int* __restrict__ cols,
                                                         const double* __restrict__ Hc, typename PEND::Tout Tout,
                                                         double* __restrict__ Ut, int N, int ld, int m, int s,
                                                         int n_strips, PEND pend) {
    extern __shared__ __attribute__((aligned(32))) double sp_smem[];
    const int m4 = (m + 3) & ~3, p = pend.p;   // (p: the constant 0 in the eager form)
    double* Hct = sp_smem;               // [s][m4]: Hct[k][a] = Hc[a][k], zero for a >= m
    double* X = Hct + s * m4;            // [s][kXS]
    double* strip = X + s * kXS;         // [p][kStrip]: the pending panel that runs along the strip
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
    [[maybe_unused]] double sv[kBatch], cv[kBatch];
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
    if constexpr (kFolds<PEND>) {
        const double* along = kind == 0 ? pend.Tq : pend.Kp;    // read at [q][base + cc]
        const double* listed = kind == 0 ? pend.Kp : pend.Tq;   // read at [q][cols[k]]
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
    }
#pragma unroll
    for (int b = 0; b < kBatch; b++) {
        if (b * kThreads >= s * kStrip) break;
        const int e = t + b * kThreads;
        int k = 0, cc = 0;
        split(e, k, cc);
        if (e < s * kStrip) X[k * kXS + cc] = v[b];
    }
    if constexpr (kFolds<PEND>) {
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
    }
    __syncthreads();

    // X[k][c] -= sum_q Kp[q][row] Tq[q][col], q ascending; wave w owns k = w, w + 4, ..
    if constexpr (kFolds<PEND>) {
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
// LDS of a candidate, in doubles: Hc [m][s] | G [s][s], T' [m][s] -- later [S | I] [m][2 m + 1] over both | 4 m + 1 of
// scratch | deferred only: fk [16][s], ft [16][s], the pending scalars of sixteen rows q.  The index lists and the control
// words of all candidates of the workgroup follow as ints.
constexpr int kFoldRows = 16;
__host__ __device__ constexpr int score_big(int m, int s) {
    return s * s + m * s > m * (2 * m + 1) ? s * s + m * s : m * (2 * m + 1);
}
__host__ __device__ constexpr int score_base_doubles(int m, int s) {
    return (m * s + score_big(m, s) + 4 * m + 1 + 1) & ~1;
}
template <class PEND>
__host__ __device__ constexpr int score_cand_doubles(int m, int s) {
    return score_base_doubles(m, s) + (kFolds<PEND> ? 2 * kFoldRows * s : 0);
}
template <class PEND>
constexpr size_t score_lds(int per, int m, int s) {
    return ((sizeof(double) * (size_t)per * score_cand_doubles<PEND>(m, s) + sizeof(int) * (size_t)per * (s + 2)) + 15) &
           ~(size_t)15;
}
constexpr int kWaveM = 16;                   // up to here a wave per candidate, LDS permitting
constexpr size_t kWaveLds = 64 * 1024;       // what four candidates of a workgroup may take together
static_assert(score_lds<Eager>(4, 16, 31) <= kWaveLds && score_lds<Eager>(4, 16, 32) > kWaveLds &&
                  score_lds<Pending>(4, 16, 22) <= kWaveLds && score_lds<Pending>(4, 16, 23) > kWaveLds,
              "where the wave form ends at m = 16: s = 31 | 32 eager, s = 22 | 23 deferred");

// NT threads per candidate, 256 / NT candidates per workgroup; EPT = elements of S per thread (m * m <= NT * EPT).
// cols [J][s], Hc [J][m][s], R [J][m][m] or [m][m], nu [J][m] or NULL with nis NULL, S_out [J][m][m] or NULL, flag [J],
// Sinv [64][64] (stride 64) or NULL: written for candidate 0 when its S is regular.
template <int NT, int EPT, class PEND>
__global__ __launch_bounds__(kThreads) void k_dsp_score(const double* __restrict__ Sigma, const int* __restrict__ cols,
                                                        const double* __restrict__ Hc, const double* __restrict__ R,
                                                        int r_shared, const double* __restrict__ nu,
                                                        double* __restrict__ nis, double* __restrict__ S_out,
                                                        int* __restrict__ flag, double* __restrict__ Sinv, int ld, int m,
                                                        int s, int J, PEND pend) {
    extern __shared__ __attribute__((aligned(32))) double sp_smem[];
    constexpr int PER = kThreads / NT;
    const int sub = threadIdx.x / NT, t = threadIdx.x % NT;
    const int cand = blockIdx.x * PER + sub;
    if (cand >= J) return;   // (uniform over the candidate's thread group; NT = 64 takes no workgroup barrier)
    const int cd = score_cand_doubles<PEND>(m, s), mm = m * m, ms = m * s, stride = 2 * m + 1;
    double* hc = sp_smem + sub * cd;     // [m][s]
    double* G = hc + ms;                 // [s][s] = Sigma_cur[cols, cols]
    double* Tl = G + s * s;              // [m][s] = Hc G
    double* M = G;                       // [m][stride], once G and T' are spent
    double* tail = G + score_big(m, s);
    int* lc = reinterpret_cast<int*>(sp_smem + PER * cd) + sub * (s + 2);
    const GjScratch sc{tail, tail + 2 * m, tail + 3 * m, tail + 4 * m, lc + s};

    for (int e = t; e < s; e += NT) lc[e] = cols[(size_t)cand * s + e];
    for (int e = t; e < ms; e += NT) hc[e] = Hc[(size_t)cand * ms + e];
    gj_sync<NT>();
    for (int e = t; e < s * s; e += NT) {   // lanes along the list: neighbouring indices share a cache line
        const int a = e / s, b = e - a * s;
        G[e] = Sigma[(size_t)lc[a] * ld + lc[b]];
    }
    gj_sync<NT>();
    if constexpr (kFolds<PEND>) {   // G[a][b] -= sum_q Kp[q][cols[a]] Tq[q][cols[b]], q ascending
        constexpr int FB = kFoldRows * kMaxS / NT;    // pending scalars of a chunk per thread and panel
        double* fk = hc + score_base_doubles(m, s);   // [kFoldRows][s]: Kp[q][cols[a]]
        double* ft = fk + kFoldRows * s;              // [kFoldRows][s]: Tq[q][cols[b]]
        const int p = pend.p;
        for (int q0 = 0; q0 < p; q0 += kFoldRows) {
            const int qs = min(kFoldRows, p - q0) * s;
            double kv[FB], tv[FB];
#pragma unroll
            for (int i = 0; i < FB; i++) {   // every load of the chunk is issued before the first is used
                if (i * NT >= qs) break;     // (uniform)
                const int e = t + i * NT;
                kv[i] = 0.0, tv[i] = 0.0;
                if (e < qs) {
                    const size_t off = (size_t)(q0 + e / s) * ld + lc[e % s];
                    kv[i] = pend.Kp[off];
                    tv[i] = pend.Tq[off];
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

template <class PEND>
hipError_t prepare(int p) {
    // gather: 64.8 KiB at m = s = 64, 128.8 KiB with p = 64 rows pending; scoring: 64 KiB for four waves, 98.8 KiB
    // (deferred 114.8 KiB) for the workgroup at m = s = 64
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dsp_gather<PEND>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)gather_lds(kMaxM, kMaxS, p));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dsp_score<64, 4, PEND>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWaveLds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dsp_score<256, 16, PEND>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)score_lds<PEND>(1, kMaxM, kMaxS));
}

template <class PEND>
void launch_score(const double* Sigma, PEND pend, const int* cols, const double* Hc, const double* R, int r_shared,
                  const double* nu, int J, int m, int s, int ld, double* nis, double* S_out, int* flag, double* Sinv,
                  hipStream_t st) {
    if (m <= kWaveM && score_lds<PEND>(4, m, s) <= kWaveLds)
        hipLaunchKernelGGL((k_dsp_score<64, 4, PEND>), dim3((J + 3) / 4), dim3(kThreads), score_lds<PEND>(4, m, s), st,
                           Sigma, cols, Hc, R, r_shared, nu, nis, S_out, flag, Sinv, ld, m, s, J, pend);
    else
        hipLaunchKernelGGL((k_dsp_score<256, 16, PEND>), dim3(J), dim3(kThreads), score_lds<PEND>(1, m, s), st, Sigma,
                           cols, Hc, R, r_shared, nu, nis, S_out, flag, Sinv, ld, m, s, J, pend);
}

// The gather and the scoring with J = 1 (S^-1 into ws, the verdict word, nis) in front of either form's gain.
template <class PEND>
void launch_panels(const Dense64CorrectPlan& pl, const double* Sigma, PEND pend, double* Tout, double* ws, const int* cols,
                   const double* Hc, const double* R, const double* nu, int m, int s, double* nis, double* S_out,
                   int* verdict, hipStream_t st) {
    // the panels are written up to N rounded up to 128 (zeros from N on): ld itself when N spans the handle, and with a live
    // dimension below it every strip the gain and the update of that width read
    const int n_strips = (pl.N + 127) / 128 * 2;
    hipLaunchKernelGGL(k_dsp_gather<PEND>, dim3(2 * n_strips), dim3(kThreads), gather_lds(m, s, pend.p), st, Sigma, cols,
                       Hc, Tout, ws + pl.off_Ut, pl.N, pl.ld, m, s, n_strips, pend);
    launch_score(Sigma, pend, cols, Hc, R, 1, nu, 1, m, s, pl.ld, nu ? nis : nullptr, S_out, verdict, ws + pl.off_Sinv,
                 st);
}

}  // namespace

hipError_t dense64_sparse_prepare() {
    const hipError_t e = prepare<Eager>(0);
    return e != hipSuccess ? e : prepare<Pending>(kMaxP);
}

void launch_dense64_score_sparse(const double* Sigma, const double* Kp, const double* Tq, int p, const int* cols,
                                 const double* Hc, const double* R, int r_shared, const double* nu, int J, int m, int s,
                                 int ld, double* nis, double* S_out, int* flag, double* Sinv, hipStream_t st) {
    if (p > 0)
        launch_score(Sigma, Pending{Kp, Tq, p}, cols, Hc, R, r_shared, nu, J, m, s, ld, nis, S_out, flag, Sinv, st);
    else
        launch_score(Sigma, Eager{}, cols, Hc, R, r_shared, nu, J, m, s, ld, nis, S_out, flag, Sinv, st);
}

void launch_dense64_correct_sparse(const Dense64CorrectPlan& pl, double* Sigma, double* state, double* ws,
                                   const int* cols, const double* Hc, const double* R, const double* nu, int m, int s,
                                   double* nis, int* verdict, hipStream_t st) {
    launch_panels(pl, Sigma, Eager{}, ws + pl.off_T, ws, cols, Hc, R, nu, m, s, nis, nullptr, verdict, st);
    launch_dense64_correct_tail(pl, Sigma, state, ws, nu, m, verdict, st);
}

void launch_dense64_sparse_panels(const Dense64CorrectPlan& pl, const double* Sigma, double* ws, const int* cols,
                                  const double* Hc, const double* R, const double* nu, int m, int s, double* nis,
                                  double* S_out, int* verdict, hipStream_t st) {
    launch_panels(pl, Sigma, Eager{}, ws + pl.off_T, ws, cols, Hc, R, nu, m, s, nis, S_out, verdict, st);
}

void launch_dense64_correct_deferred(const Dense64CorrectPlan& pl, const double* Sigma, double* state, double* ws,
                                     double* Kp, double* Tq, int p, const int* cols, const double* Hc, const double* R,
                                     const double* nu, int m, int s, double* nis, int* verdict, hipStream_t st) {
    launch_panels(pl, Sigma, Pending{Kp, Tq, p}, Tq + (size_t)p * pl.ld, ws, cols, Hc, R, nu, m, s, nis, nullptr, verdict,
                  st);
    launch_dense64_gain(pl, ws, Kp + (size_t)p * pl.ld, state, nu, m, verdict, st);
}

}  // namespace ekf
