// ekf_dense64_value.hip -- which landmark is worth looking at next: for every landmark of a range, what a hypothetical
// range-bearing observation of it would take off the trace of Sigma, off the pose variances and off the entropy of the
// dense fp64 handle's map, before any reading has arrived (gfx950, wave64).  With H the m = 2 Jacobian of landmark i (five
// non-zero columns: the pose and the landmark's own pair), U = Sigma H^T and S = H Sigma H^T + R the drops are
// tr(S^-1 U^T U), tr(S^-1 U_p^T U_p) (U_p: rows 0 .. 2) and 0.5 (log det S - log det R).  Row r of U for landmark i needs
// Sigma[r][0 .. 2] and Sigma[r][3 + 2 i .. 4 + 2 i] only, so ALL landmarks together read every element of the live corner
// exactly once, along rows.  The definitions are include/ekfslam.h's.
//   k_dv_terms    the model call only, one thread per landmark: cols, Hc (measurement_terms of ekf_kernels.hpp: the
//                 reference's Hj depends on pose and landmark alone, the reading is any), the shared R, and in_view from the
//                 predicted range.
//   k_dv_cols     the operands call only: cols.
//   (S and flag are ONE launch of k_dsp_score, ekf_dense64_sparse.hip, on these operands: the sparse scoring's own bits.)
//   k_dv_tile     a short-lived workgroup per tile of kDense64ValueTileRows rows x kDense64ValueTileLm landmarks, lane =
//                 landmark: a wave's 16-byte loads (landmark columns start at the odd index 3: pair8) run along a row of
//                 Sigma, 1 KiB contiguous.  The three pose entries of the tile's rows go through LDS once (broadcast reads),
//                 Hc sits in registers.  Per row r: u[a] = sum_k Sigma[r][cols[k]] Hc[a][k] from +0 in ascending k, then
//                 g00 += u0 u0, g01 += u0 u1, g11 += u1 u1 in ascending r, every product and sum rounded on its own; rows
//                 0 .. 2 go into a second triple as well.  Eight rows' loads are issued before the first is used.  Loads are
//                 masked at Na and at count: nothing at an index >= Na is read.  One record of six doubles per (row tile,
//                 landmark), component-major so that the stores and the fold's loads run along the landmarks.
//   k_dv_fold     a workgroup per 32 landmarks: 192 threads sum the records in ascending row-tile order (the pose triple
//                 lives in row tile 0 alone), then each wave takes its landmarks one after the other: [S | I] into LDS,
//                 gj_invert of ekf_dense64_invert.hpp (the sparse scoring's routine on the sparse scoring's S, so its
//                 verdict is that call's flag), and on lane 0 the two traces and det S; NaN for a flagged landmark.
//   k_dv_best     one workgroup: the largest dtrace, dtrace_pose and det S among the landmarks with flag = 0 and
//                 in_view = 1, "larger value, then lower index, a NaN never": a pure function of the data, the same at
//                 every level of the reduction (the max twin of lm_block_min, ekf_dense64_lm.hpp).
// THE ORDER OF SUMMATION is a function of Na and kDense64ValueTileRows alone: ascending rows inside a row tile, then
// ascending tiles.  So a landmark's figures do not depend on first_lm / count, on the capacity of the handle or on the run.
// No floating-point atomics, no waits inside a kernel.
#include "ekf_dense64_invert.hpp"
#include "ekf_dense64_lm.hpp"

namespace ekf {

namespace {

using lm::pair16;
using lm::pair8;

constexpr int kRows = kDense64ValueTileRows;
constexpr int kLm = kDense64ValueTileLm;
constexpr int kThreads = kDense64ValueThreads;
constexpr int kAhead = 8;            // rows whose loads are in flight together
constexpr int kFoldThreads = 256;
constexpr int kFoldLm = 32;          // landmarks of a fold workgroup
constexpr int kFoldWaves = kFoldThreads / 64;
constexpr int kGjDoubles = 20;       // [S | I] [2][5] | prow [4] | fcol [2] | wv [2] | pv [1], rounded up to even
static_assert(kLm == kThreads && kRows % kAhead == 0 && 6 * kFoldLm <= kFoldThreads, "lane = landmark; a thread per sum");

__device__ __forceinline__ void store_hc(double* __restrict__ Hc, int c, const double (&H)[2][5]) {
    pair16* h = reinterpret_cast<pair16*>(Hc + (size_t)c * 10);   // 80 bytes per candidate on a 16-byte base
    h[0] = pair16{H[0][0], H[0][1]};
    h[1] = pair16{H[0][2], H[0][3]};
    h[2] = pair16{H[0][4], H[1][0]};
    h[3] = pair16{H[1][1], H[1][2]};
    h[4] = pair16{H[1][3], H[1][4]};
}

__device__ __forceinline__ void store_cols(int* __restrict__ cols, int c, int i) {
    int* cc = cols + (size_t)c * 5;
    cc[0] = 0; cc[1] = 1; cc[2] = 2; cc[3] = 3 + 2 * i; cc[4] = 4 + 2 * i;
}

__global__ __launch_bounds__(lm::kLmThreads) void k_dv_terms(const double* __restrict__ state, int first_lm, int count,
                                                             double r_meas, double range_max, int* __restrict__ cols,
                                                             double* __restrict__ Hc, double* __restrict__ R,
                                                             unsigned char* __restrict__ in_view) {
    const int j = blockIdx.x * lm::kLmThreads + threadIdx.x, lane = threadIdx.x & 63;
    const double pv = state[lane < 3 ? lane : 0];   // three lanes load the pose, the wave takes it through the scalar file
    const double theta = lane_bcast(pv, 0), x = lane_bcast(pv, 1), y = lane_bcast(pv, 2);
    if (j == 0) {
        R[0] = r_meas; R[1] = 0.0; R[2] = 0.0; R[3] = r_meas;   // :172-175, shared by the landmarks
    }
    if (j >= count) return;
    const int i = first_lm + j;
    const pair8 t = *reinterpret_cast<const pair8*>(state + 3 + 2 * i);
    MeasTerms m;
    measurement_terms(t.x, t.y, 1.0, 0.0, theta, x, y, m);   // Hj (:158-166) and the predicted range do not see the reading
    store_hc(Hc, j, m.H);
    store_cols(cols, j, i);
    in_view[j] = range_max > 0.0 ? (m.zh0 <= range_max ? 1 : 0) : 1;   // (a NaN range is not in view)
}

__global__ __launch_bounds__(lm::kLmThreads) void k_dv_cols(int first_lm, int count, int* __restrict__ cols) {
    const int j = blockIdx.x * lm::kLmThreads + threadIdx.x;
    if (j < count) store_cols(cols, j, first_lm + j);
}

// rec [row_tiles][6][count]: g00, g01, g11 of the tile's rows, then the same of rows 0 .. 2 (zero from row tile 1 on)
__global__ __launch_bounds__(kThreads) void k_dv_tile(const double* __restrict__ S, int ld, int Na, int first_lm, int count,
                                                      const double* __restrict__ Hc, double* __restrict__ rec) {
    __shared__ double ps[3 * kRows];
    const int t = threadIdx.x, j = kLm * blockIdx.x + t, r0 = kRows * blockIdx.y;
    const int nr = min(kRows, Na - r0);
    for (int e = t; e < 3 * nr; e += kThreads) ps[e] = S[(size_t)(r0 + e / 3) * ld + e % 3];
    __syncthreads();
    if (j >= count) return;
    const pair16* hp = reinterpret_cast<const pair16*>(Hc + (size_t)j * 10);
    const pair16 q0 = hp[0], q1 = hp[1], q2 = hp[2], q3 = hp[3], q4 = hp[4];
    const double h[2][5] = {{q0.x, q0.y, q1.x, q1.y, q2.x}, {q2.y, q3.x, q3.y, q4.x, q4.y}};
    const double* col = S + (size_t)r0 * ld + 3 + 2 * (first_lm + j);   // (3 + 2 (first_lm + count) <= Na)
    double g00 = 0.0, g01 = 0.0, g11 = 0.0, p00 = 0.0, p01 = 0.0, p11 = 0.0;
    for (int rb = 0; rb < nr; rb += kAhead) {
        pair8 v[kAhead];
#pragma unroll
        for (int u = 0; u < kAhead; u++) {
            v[u] = pair8{0.0, 0.0};
            if (rb + u < nr) v[u] = *reinterpret_cast<const pair8*>(col + (size_t)(rb + u) * ld);
        }
#pragma unroll
        for (int u = 0; u < kAhead; u++) {
            if (rb + u >= nr) break;   // (uniform)
            const double s[5] = {ps[3 * (rb + u)], ps[3 * (rb + u) + 1], ps[3 * (rb + u) + 2], v[u].x, v[u].y};
            double w[2];
#pragma unroll
            for (int a = 0; a < 2; a++) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 5; k++) acc = acc + s[k] * h[a][k];
                w[a] = acc;
            }
            const double a00 = w[0] * w[0], a01 = w[0] * w[1], a11 = w[1] * w[1];
            g00 = g00 + a00; g01 = g01 + a01; g11 = g11 + a11;
            if (r0 + rb + u < 3) {   // (uniform) the pose rows
                p00 = p00 + a00; p01 = p01 + a01; p11 = p11 + a11;
            }
        }
    }
    double* out = rec + (size_t)blockIdx.y * 6 * count + j;
    out[0] = g00;
    out[(size_t)count] = g01;
    out[(size_t)2 * count] = g11;
    out[(size_t)3 * count] = p00;
    out[(size_t)4 * count] = p01;
    out[(size_t)5 * count] = p11;
}

// fl-chain a00 g00 + a01 g01 + a10 g01 + a11 g11, in that order
__device__ __forceinline__ double trace_of(const double (&A)[4], double g00, double g01, double g11) {
    double v = A[0] * g00;
    v = v + A[1] * g01;
    v = v + A[2] * g01;
    v = v + A[3] * g11;
    return v;
}

__global__ __launch_bounds__(kFoldThreads) void k_dv_fold(const double* __restrict__ rec, int row_tiles, int count,
                                                          const double* __restrict__ S, double* __restrict__ dtrace,
                                                          double* __restrict__ dpose, double* __restrict__ detS) {
    __shared__ double Gs[6][kFoldLm];
    __shared__ __attribute__((aligned(16))) double gj[kFoldWaves][kGjDoubles];
    __shared__ int ctl[kFoldWaves][2];
    const int tid = threadIdx.x, c0 = kFoldLm * blockIdx.x;
    if (tid < 6 * kFoldLm) {
        const int comp = tid / kFoldLm, l = tid % kFoldLm;
        double acc = 0.0;
        if (c0 + l < count) {
            const double* p = rec + (size_t)comp * count + c0 + l;
            const int tiles = comp < 3 ? row_tiles : 1;   // rows 0 .. 2 lie in row tile 0
            for (int k = 0; k < tiles; k++) acc = acc + p[(size_t)k * 6 * count];
        }
        Gs[comp][l] = acc;
    }
    __syncthreads();
    const int w = tid >> 6, t = tid & 63;
    double* M = gj[w];   // [2][5]
    const GjScratch sc{M + 10, M + 14, M + 16, M + 18, ctl[w]};
    const double nan = __builtin_nan("");
    for (int l = w; l < kFoldLm; l += kFoldWaves) {
        const int cand = c0 + l;
        if (cand >= count) break;   // (uniform over the wave; only wave-level barriers from here on)
        int bad = 0;
        double sv = 0.0;
        if (t < 4) {
            sv = S[(size_t)cand * 4 + t];
            const int a = t >> 1, b = t & 1;
            if (!isfinite(sv)) bad = 1;
            M[a * 5 + b] = sv;
            M[a * 5 + 2 + b] = a == b ? 1.0 : 0.0;
        }
        const int verdict = gj_invert<64>(M, 5, sc, 2, t, bad);
        if (t == 0) {
            double dt = nan, dp = nan, det = nan;
            if (!verdict) {
                const double A[4] = {M[2], M[3], M[7], M[8]};
                dt = trace_of(A, Gs[0][l], Gs[1][l], Gs[2][l]);
                dp = trace_of(A, Gs[3][l], Gs[4][l], Gs[5][l]);
                const double s00 = S[(size_t)cand * 4], s01 = S[(size_t)cand * 4 + 1], s10 = S[(size_t)cand * 4 + 2],
                             s11 = S[(size_t)cand * 4 + 3];
                det = s00 * s11 - s01 * s10;
            }
            dtrace[cand] = dt;
            dpose[cand] = dp;
            detS[cand] = det;
        }
        gj_sync<64>();   // lane 0 is done with M before the wave's next landmark overwrites it
    }
}

// (value, index) order of the winners: the larger value, then the lower index
struct Top {
    double v;
    int i;
};
__device__ __forceinline__ void top_take(Top& t, double ov, int oi) {
    if (ov > t.v || (ov == t.v && oi < t.i)) { t.v = ov; t.i = oi; }
}

__global__ __launch_bounds__(lm::kLmThreads) void k_dv_best(const double* __restrict__ dtrace, const double* __restrict__ dpose,
                                                            const double* __restrict__ detS, const int* __restrict__ flag,
                                                            const unsigned char* __restrict__ in_view, int count,
                                                            Dense64ValueBest* __restrict__ best) {
    __shared__ Top sh[3][lm::kLmThreads / 64];
    const int tid = threadIdx.x;
    const double* val[3] = {dtrace, dpose, detS};
    Top top[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        Top t{-__builtin_huge_val(), 0x7fffffff};
        for (int j = tid; j < count; j += lm::kLmThreads) {
            const double v = val[c][j];
            if (flag[j] == 0 && in_view[j] != 0 && v == v) top_take(t, v, j);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double ov = __shfl_xor(t.v, off, 64);
            const int oi = __shfl_xor(t.i, off, 64);
            top_take(t, ov, oi);
        }
        if ((tid & 63) == 0) sh[c][tid >> 6] = t;
        top[c] = t;
    }
    __syncthreads();
    if (tid != 0) return;
#pragma unroll
    for (int c = 0; c < 3; c++)
        for (int w = 1; w < lm::kLmThreads / 64; w++) top_take(top[c], sh[c][w].v, sh[c][w].i);
    const double nan = __builtin_nan("");
    const bool h0 = top[0].i != 0x7fffffff, h1 = top[1].i != 0x7fffffff, h2 = top[2].i != 0x7fffffff;
    best->i_trace = h0 ? top[0].i : -1;
    best->i_pose = h1 ? top[1].i : -1;
    best->i_det = h2 ? top[2].i : -1;
    best->reserved = 0;
    best->v_trace = h0 ? top[0].v : nan;
    best->v_pose = h1 ? top[1].v : nan;
    best->v_det = h2 ? top[2].v : nan;
}

constexpr size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

}  // namespace

Dense64ValuePlan dense64_value_plan(int Na, int first_lm, int count) {
    Dense64ValuePlan p{};
    p.Na = Na;
    p.first_lm = first_lm;
    p.count = count;
    p.row_tiles = (Na + kRows - 1) / kRows;
    p.lm_tiles = (count + kLm - 1) / kLm;
    const size_t n = (size_t)count;
    p.off_Hc = 0;
    p.off_R = p.off_Hc + sizeof(double) * 10 * n;
    p.off_S = p.off_R + sizeof(double) * 4;
    p.off_dtrace = p.off_S + sizeof(double) * 4 * n;
    p.off_dpose = up16(p.off_dtrace + sizeof(double) * n);
    p.off_det = up16(p.off_dpose + sizeof(double) * n);
    p.off_best = up16(p.off_det + sizeof(double) * n);
    p.off_rec = p.off_best + up16(sizeof(Dense64ValueBest));
    p.off_cols = up16(p.off_rec + sizeof(double) * 6 * n * p.row_tiles);
    p.off_flag = up16(p.off_cols + sizeof(int) * 5 * n);
    p.off_view = up16(p.off_flag + sizeof(int) * n);
    p.bytes = up16(p.off_view + n);
    return p;
}

void launch_dense64_value_terms(const Dense64ValuePlan& p, const double* state, double r_meas, double range_max, void* ws,
                                hipStream_t st) {
    char* b = static_cast<char*>(ws);
    hipLaunchKernelGGL(k_dv_terms, dim3((p.count + lm::kLmThreads - 1) / lm::kLmThreads), dim3(lm::kLmThreads), 0, st, state,
                       p.first_lm, p.count, r_meas, range_max, reinterpret_cast<int*>(b + p.off_cols),
                       reinterpret_cast<double*>(b + p.off_Hc), reinterpret_cast<double*>(b + p.off_R),
                       reinterpret_cast<unsigned char*>(b + p.off_view));
}

void launch_dense64_value_cols(const Dense64ValuePlan& p, void* ws, hipStream_t st) {
    hipLaunchKernelGGL(k_dv_cols, dim3((p.count + lm::kLmThreads - 1) / lm::kLmThreads), dim3(lm::kLmThreads), 0, st,
                       p.first_lm, p.count, reinterpret_cast<int*>(static_cast<char*>(ws) + p.off_cols));
}

void launch_dense64_value(const Dense64ValuePlan& p, const double* Sigma, int ld, void* ws, hipStream_t st) {
    char* b = static_cast<char*>(ws);
    const int* cols = reinterpret_cast<const int*>(b + p.off_cols);
    const double* Hc = reinterpret_cast<const double*>(b + p.off_Hc);
    double* S = reinterpret_cast<double*>(b + p.off_S);
    double* rec = reinterpret_cast<double*>(b + p.off_rec);
    double* dtrace = reinterpret_cast<double*>(b + p.off_dtrace);
    double* dpose = reinterpret_cast<double*>(b + p.off_dpose);
    double* det = reinterpret_cast<double*>(b + p.off_det);
    int* flag = reinterpret_cast<int*>(b + p.off_flag);
    launch_dense64_score_sparse(Sigma, nullptr, nullptr, 0, cols, Hc, reinterpret_cast<const double*>(b + p.off_R), 1, nullptr,
                                p.count, 2, 5, ld, nullptr, S, flag, nullptr, st);
    hipLaunchKernelGGL(k_dv_tile, dim3(p.lm_tiles, p.row_tiles), dim3(kThreads), 0, st, Sigma, ld, p.Na, p.first_lm, p.count,
                       Hc, rec);
    hipLaunchKernelGGL(k_dv_fold, dim3((p.count + kFoldLm - 1) / kFoldLm), dim3(kFoldThreads), 0, st, rec, p.row_tiles,
                       p.count, S, dtrace, dpose, det);
    hipLaunchKernelGGL(k_dv_best, dim3(1), dim3(lm::kLmThreads), 0, st, dtrace, dpose, det, flag,
                       reinterpret_cast<const unsigned char*>(b + p.off_view), p.count, reinterpret_cast<Dense64ValueBest*>(b + p.off_best));
}

}  // namespace ekf
