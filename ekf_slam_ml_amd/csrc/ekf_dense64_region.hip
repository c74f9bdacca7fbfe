// ekf_dense64_region.hip -- a local region of the dense fp64 handle: the compressed EKF of Guivant & Nebot (2001) on the
// handle's own Sigma.  While a region A = [0, Na) is open the structured calls run at live dimension Na on Sigma_aa and x_a
// as they always do, and three accumulators record what the rest B = [Na, N) of the map will owe (Sigma0 = Sigma as stored
// at region_begin; Phi = I, Psi = 0, theta = 0 there):
//   Sigma_ab = Phi Sigma0_ab    Sigma_ba = Sigma0_ba Phi^T    Sigma_bb = Sigma0_bb - Sigma0_ba Psi Sigma0_ab
//   x_b = x0_b + Sigma0_ba theta
// (plan and layout: ekf_dense64_region.hpp; the algebra: DESIGN.md 4.8.21).
//   k_dr_panels   a correction's panels from the Phi BEFORE the call: W = Hc Phi[cols, :] (m x Na), Z = S^-1 W, and
//                 theta += Z^T nu; a workgroup per 32 columns, everything of a column stays in the workgroup.
//   k_dr_update   Phi -= K_a W and Psi += W^T Z in one streaming pass over tiles of 32 x 64 of the Na x Na pair: 32 Na^2
//                 bytes per correction.  K_a^T [m][ld] is the panel the live call's gain left (the workspace, or the pending
//                 rows of a deferred call); S^-1 and nu are the live call's too.
//   k_dr_rowmap   Phi[b, :] <- M Phi[src, :] for propagate_block (src = b itself) and init_block (src = cols; zeros at
//                 s = 0): a thread per column, all loads of a column before its stores.
//   k_dr_state    x_b += Sigma0_ba theta, a thread per row of B.
//   k_dr_project  Y = -(Psi Sigma0_ab) and V = Phi Sigma0_ab into the scratch, [Na][ld] each, columns outside [Na, N) zero.
//   k_dr_sbb      Sigma_bb += Sigma0_ba Y on gemm_tile<double> of ekf_dense_gemm.hpp, a workgroup per 128 x 128 tile of
//                 Sigma's own grid from the tile that holds Na on, K = Na rounded up to BK = 16.  A is Sigma itself
//                 (rows >= Na, columns < Na), so the K range behind Na and the rows of a tile in front of Na hold REAL
//                 entries of Sigma_bb and Sigma_aa: RegionMask answers with zeros for them at the load and keeps every
//                 entry with a row or column index < Na or >= N from being read or stored at all.
//   k_dr_bat      (Sigma0_ba Phi^T)^T into the scratch Y (dead by then), through an LDS transpose of Sigma0_ba.
//   k_dr_put_ba   Sigma_ba <- that, transposed back;  k_dr_put_ab   Sigma_ab <- V.
// Every kernel of a call in a region reads the call's verdict word first and does nothing when the correction refused.
// Order of arithmetic: every sum in ascending index from +0 (or from the stored value where it updates in place), one fused
// multiply-add per term, written fma() because the library is built with -ffp-contract=off; no atomics; nothing before
// region_end depends on N or ld.  The one exception is k_dr_sbb: the MFMA takes its four k of a step in the order of the
// instruction, the steps in ascending k.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense_gemm.hpp"

namespace ekf {

namespace {

constexpr int kThreads = kDense64RegionThreads;
constexpr int kMaxM = kDense64MaxM, kMaxS = kDense64MaxS;
constexpr int kPC = kDense64RegionPanelCols;
constexpr int kTR = kDense64RegionTileRows, kTC = kDense64RegionTileCols;

// W [m][pitch], Z [m][pitch], theta [pitch]; Phi [Na][pitch]; Sinv [64][64]; nu: m or NULL (theta untouched)
__global__ __launch_bounds__(kThreads) void k_dr_panels(const double* __restrict__ Phi, const int* __restrict__ cols,
                                                        const double* __restrict__ Hc, const double* __restrict__ Sinv,
                                                        const double* __restrict__ nu, const int* __restrict__ verdict,
                                                        double* __restrict__ W, double* __restrict__ Z,
                                                        double* __restrict__ theta, int Na, int pitch, int m, int s) {
    __shared__ double Wl[kMaxM][kPC + 1], Zl[kMaxM][kPC + 1];
    if (*verdict != 0) return;   // (uniform)
    const int c = threadIdx.x % kPC, g = threadIdx.x / kPC, j = blockIdx.x * kPC + c;
    constexpr int G = kThreads / kPC;
    const bool real = j < Na;
    for (int a = g; a < m; a += G) {
        double acc = 0.0;
        if (real)
            for (int k = 0; k < s; k++) acc = fma(Hc[a * s + k], Phi[(size_t)cols[k] * pitch + j], acc);
        Wl[a][c] = acc;
        if (real) W[(size_t)a * pitch + j] = acc;
    }
    __syncthreads();
    for (int a = g; a < m; a += G) {
        double acc = 0.0;
        for (int b = 0; b < m; b++) acc = fma(Sinv[a * kMaxM + b], Wl[b][c], acc);
        Zl[a][c] = acc;
        if (real) Z[(size_t)a * pitch + j] = acc;
    }
    __syncthreads();
    if (nu && g == 0 && real) {
        double t = theta[j];
        for (int a = 0; a < m; a++) t = fma(Zl[a][c], nu[a], t);
        theta[j] = t;
    }
}

// a thread owns column j of the tile and kTR / 4 rows; the operands at the rows are uniform over a wave
__global__ __launch_bounds__(kThreads) void k_dr_update(double* __restrict__ Phi, double* __restrict__ Psi,
                                                        const double* __restrict__ Kt, const double* __restrict__ W,
                                                        const double* __restrict__ Z, const int* __restrict__ verdict,
                                                        int Na, int pitch, int ldk, int m) {
    if (*verdict != 0) return;   // (uniform)
    constexpr int RPT = kTR / (kThreads / kTC);
    const int c = threadIdx.x % kTC, g = threadIdx.x / kTC;
    const int j = blockIdx.x * kTC + c, i0 = blockIdx.y * kTR + g * RPT;
    if (j >= Na) return;   // masked element by element: nothing between Na and the tile's edge is read or written
    double phi[RPT], psi[RPT];
#pragma unroll
    for (int r = 0; r < RPT; r++) {
        const bool on = i0 + r < Na;
        phi[r] = on ? Phi[(size_t)(i0 + r) * pitch + j] : 0.0;
        psi[r] = on ? Psi[(size_t)(i0 + r) * pitch + j] : 0.0;
    }
    for (int a = 0; a < m; a++) {
        const double wj = W[(size_t)a * pitch + j], zj = Z[(size_t)a * pitch + j];
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            if (i0 + r >= Na) continue;
            phi[r] = fma(-Kt[(size_t)a * ldk + i0 + r], wj, phi[r]);
            psi[r] = fma(W[(size_t)a * pitch + i0 + r], zj, psi[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < RPT; r++)
        if (i0 + r < Na) {
            Phi[(size_t)(i0 + r) * pitch + j] = phi[r];
            Psi[(size_t)(i0 + r) * pitch + j] = psi[r];
        }
}

// Phi[first + a][j] = sum_k M[a][k] Phi[src ? src[k] : first + k][j]; s = 0 writes +0
__global__ __launch_bounds__(kThreads) void k_dr_rowmap(double* __restrict__ Phi, const double* __restrict__ M,
                                                        const int* __restrict__ src, int Na, int pitch, int first, int r,
                                                        int s) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j >= Na) return;
    double v[kMaxS];
#pragma unroll
    for (int k = 0; k < kMaxS; k++) v[k] = k < s ? Phi[(size_t)(src ? src[k] : first + k) * pitch + j] : 0.0;
    for (int a = 0; a < r; a++) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < kMaxS; k++)
            if (k < s) acc = fma(M[a * s + k], v[k], acc);
        Phi[(size_t)(first + a) * pitch + j] = acc;
    }
}

// Phi = I, Psi = 0, theta = 0 over the whole buffers (the padding too)
__global__ __launch_bounds__(kThreads) void k_dr_reset(double* __restrict__ Phi, double* __restrict__ Psi,
                                                       double* __restrict__ theta, int Na, int pitch) {
    const size_t e = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (size_t)Na * pitch) return;
    const int i = (int)(e / pitch), j = (int)(e - (size_t)i * pitch);
    Phi[e] = i == j ? 1.0 : 0.0;
    Psi[e] = 0.0;
    if (i == 0) theta[j] = 0.0;
}

__global__ __launch_bounds__(kThreads) void k_dr_state(const double* __restrict__ S, const double* __restrict__ theta,
                                                       double* __restrict__ x, int Na, int N, int ld) {
    const int i = Na + blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    double acc = x[i];
    const double* row = S + (size_t)i * ld;
    for (int k = 0; k < Na; k++) acc = fma(row[k], theta[k], acc);
    x[i] = acc;
}

// a thread owns column j and RP rows k of both panels; Sigma0_ab[l][j] is read once per row group
constexpr int kRP = 8;
__global__ __launch_bounds__(kThreads) void k_dr_project(const double* __restrict__ S, const double* __restrict__ Phi,
                                                         const double* __restrict__ Psi, double* __restrict__ Y,
                                                         double* __restrict__ V, int Na, int N, int ld, int pitch) {
    const int j = blockIdx.x * kThreads + threadIdx.x, k0 = blockIdx.y * kRP;
    if (j >= ld) return;
    const bool real = j >= Na && j < N;
    double y[kRP], v[kRP];
#pragma unroll
    for (int r = 0; r < kRP; r++) y[r] = 0.0, v[r] = 0.0;
    if (real)
        for (int l = 0; l < Na; l++) {
            const double x = S[(size_t)l * ld + j];
#pragma unroll
            for (int r = 0; r < kRP; r++) {
                if (k0 + r >= Na) continue;
                y[r] = fma(Psi[(size_t)(k0 + r) * pitch + l], x, y[r]);
                v[r] = fma(Phi[(size_t)(k0 + r) * pitch + l], x, v[r]);
            }
        }
#pragma unroll
    for (int r = 0; r < kRP; r++)
        if (k0 + r < Na) {
            Y[(size_t)(k0 + r) * ld + j] = real ? -y[r] : 0.0;   // the negation is exact: Sigma_bb + Sigma0_ba Y
            V[(size_t)(k0 + r) * ld + j] = real ? v[r] : 0.0;
        }
}

// what k_dr_sbb hangs on the tile: A = Sigma (rows of B, columns of A), B = Y [Na][ld], C = Qadd = Sigma
struct RegionMask {
    static constexpr bool kOn = true;
    int Na, N;
    __device__ __forceinline__ f64x2 a(const double* p, int row, int k) const {
        f64x2 v = {0.0, 0.0};
        if (row >= Na && row < N) {
            if (k < Na) v[0] = p[0];
            if (k + 1 < Na) v[1] = p[1];
        }
        return v;
    }
    __device__ __forceinline__ f64x2 b(const double* p, int k, int col) const {
        f64x2 v = {0.0, 0.0};
        if (k < Na) {   // (Y has Na rows: nothing behind them is addressed)
            if (col >= Na && col < N) v[0] = p[0];
            if (col + 1 >= Na && col + 1 < N) v[1] = p[1];
        }
        return v;
    }
    __device__ __forceinline__ bool c(int row, int col) const { return row >= Na && row < N && col >= Na && col < N; }
};

// A, C and Qadd of the tile are all Sigma, and gemm_tile declares them __restrict__.  What is read through A (rows >= Na,
// columns < Na: Sigma0_ba; everything else of a row is answered by the mask without a load) and what is written through C
// (rows and columns >= Na: Sigma_bb) are disjoint sets of entries, so no load through A can see a store of this launch --
// from this workgroup or another.  Qadd and C are the same entry only within one thread, which loads it, adds and stores
// it, in that order (the trailing update of ekf_dense64_factor.hip uses the tile the same way).
using SbbTile = GemmMainTile<double, false>;
__global__ __launch_bounds__(kThreads, 2) void k_dr_sbb(double* S, const double* __restrict__ Y, int Na, int N, int ld,
                                                        int tile0, int gemm_k) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dr_smem[];
    const int row0 = (tile0 + (int)blockIdx.y) * SbbTile::TM, col0 = (tile0 + (int)blockIdx.x) * SbbTile::TN;
    gemm_tile<double, false, SbbTile::NBUF, SbbTile::WTM, SbbTile::WTN, RegionMask>(
        S, Y, S, S, ld, row0, col0, reinterpret_cast<double*>(dr_smem), gemm_k, RegionMask{Na, N});
}

// Wt[k][i] = sum_l Sigma0[i][l] Phi[k][l] for 64 rows i of B and 32 rows k of Phi per workgroup, l ascending in chunks of
// 64 that go through LDS (loaded along rows of Sigma, read along its columns)
constexpr int kBK = 32;
__global__ __launch_bounds__(kThreads) void k_dr_bat(const double* __restrict__ S, const double* __restrict__ Phi,
                                                     double* __restrict__ Wt, int Na, int N, int ld, int pitch) {
    __shared__ double X[64][65];
    constexpr int RPT = kBK / 4;
    const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int i0 = Na + blockIdx.x * 64, k0 = blockIdx.y * kBK + g * RPT;
    double acc[RPT];
#pragma unroll
    for (int r = 0; r < RPT; r++) acc[r] = 0.0;
    for (int l0 = 0; l0 < Na; l0 += 64) {
        __syncthreads();
        for (int e = threadIdx.x; e < 64 * 64; e += kThreads) {
            const int ii = e >> 6, ll = e & 63;
            X[ii][ll] = (i0 + ii < N && l0 + ll < Na) ? S[(size_t)(i0 + ii) * ld + l0 + ll] : 0.0;
        }
        __syncthreads();
        const int nl = min(64, Na - l0);
        for (int ll = 0; ll < nl; ll++) {
            const double x = X[c][ll];
#pragma unroll
            for (int r = 0; r < RPT; r++)
                if (k0 + r < Na) acc[r] = fma(x, Phi[(size_t)(k0 + r) * pitch + l0 + ll], acc[r]);
        }
    }
    if (i0 + c < N)
#pragma unroll
        for (int r = 0; r < RPT; r++)
            if (k0 + r < Na) Wt[(size_t)(k0 + r) * ld + i0 + c] = acc[r];
}

// Sigma[i][k] = Wt[k][i], i in [Na, N), k < Na: 64 x 64 tiles through LDS
__global__ __launch_bounds__(kThreads) void k_dr_put_ba(double* __restrict__ S, const double* __restrict__ Wt, int Na, int N,
                                                        int ld) {
    __shared__ double X[64][65];
    const int i0 = Na + blockIdx.x * 64, k0 = blockIdx.y * 64;
    for (int e = threadIdx.x; e < 64 * 64; e += kThreads) {
        const int kk = e >> 6, ii = e & 63;
        X[kk][ii] = (k0 + kk < Na && i0 + ii < N) ? Wt[(size_t)(k0 + kk) * ld + i0 + ii] : 0.0;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * 64; e += kThreads) {
        const int ii = e >> 6, kk = e & 63;
        if (k0 + kk < Na && i0 + ii < N) S[(size_t)(i0 + ii) * ld + k0 + kk] = X[kk][ii];
    }
}

__global__ __launch_bounds__(kThreads) void k_dr_put_ab(double* __restrict__ S, const double* __restrict__ V, int Na, int N,
                                                        int ld) {
    const int j = Na + blockIdx.x * kThreads + threadIdx.x, k = blockIdx.y;
    if (j < N) S[(size_t)k * ld + j] = V[(size_t)k * ld + j];
}

}  // namespace

hipError_t dense64_region_prepare() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dr_sbb), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)SbbTile::kLdsBytes);
}

void launch_dense64_region_reset(const Dense64RegionPlan& p, void* acc, hipStream_t st) {
    char* b = static_cast<char*>(acc);
    const size_t n = (size_t)p.Na * p.pitch;
    hipLaunchKernelGGL(k_dr_reset, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       reinterpret_cast<double*>(b + p.off_phi), reinterpret_cast<double*>(b + p.off_psi),
                       reinterpret_cast<double*>(b + p.off_theta), p.Na, p.pitch);
}

void launch_dense64_region_correct(const Dense64RegionPlan& p, void* acc, const double* Kt, int ldk, const double* Sinv,
                                   const int* cols, const double* Hc, const double* nu, int m, int s, const int* verdict,
                                   hipStream_t st) {
    char* b = static_cast<char*>(acc);
    double *Phi = reinterpret_cast<double*>(b + p.off_phi), *Psi = reinterpret_cast<double*>(b + p.off_psi);
    double *W = reinterpret_cast<double*>(b + p.off_W), *Z = reinterpret_cast<double*>(b + p.off_Z);
    hipLaunchKernelGGL(k_dr_panels, dim3(p.panel_groups), dim3(kThreads), 0, st, Phi, cols, Hc, Sinv, nu, verdict, W, Z,
                       reinterpret_cast<double*>(b + p.off_theta), p.Na, p.pitch, m, s);
    hipLaunchKernelGGL(k_dr_update, dim3(p.upd_tiles_c, p.upd_tiles_r), dim3(kThreads), 0, st, Phi, Psi, Kt, W, Z, verdict,
                       p.Na, p.pitch, ldk, m);
}

void launch_dense64_region_rowmap(const Dense64RegionPlan& p, void* acc, const double* M, const int* src, int first, int r,
                                  int s, hipStream_t st) {
    hipLaunchKernelGGL(k_dr_rowmap, dim3(p.map_groups), dim3(kThreads), 0, st,
                       reinterpret_cast<double*>(static_cast<char*>(acc) + p.off_phi), M, src, p.Na, p.pitch, first, r, s);
}

void launch_dense64_region_end(const Dense64RegionPlan& p, double* Sigma, double* state, const void* acc, void* scratch,
                               hipStream_t st) {
    const char* b = static_cast<const char*>(acc);
    const double *Phi = reinterpret_cast<const double*>(b + p.off_phi), *Psi = reinterpret_cast<const double*>(b + p.off_psi);
    const double* theta = reinterpret_cast<const double*>(b + p.off_theta);
    double* Y = reinterpret_cast<double*>(static_cast<char*>(scratch) + p.off_Y);
    double* V = reinterpret_cast<double*>(static_cast<char*>(scratch) + p.off_V);
    const int Na = p.Na, N = p.N, ld = p.ld;
    const unsigned nb_groups = (unsigned)((p.nb + kThreads - 1) / kThreads), nb_strips = (unsigned)((p.nb + 63) / 64);
    hipLaunchKernelGGL(k_dr_state, dim3(nb_groups), dim3(kThreads), 0, st, Sigma, theta, state, Na, N, ld);
    hipLaunchKernelGGL(k_dr_project, dim3((unsigned)(ld / kThreads + (ld % kThreads ? 1 : 0)), (unsigned)((Na + kRP - 1) / kRP)),
                       dim3(kThreads), 0, st, Sigma, Phi, Psi, Y, V, Na, N, ld, p.pitch);
    hipLaunchKernelGGL(k_dr_sbb, dim3(p.gemm_tiles, p.gemm_tiles), dim3(kThreads), SbbTile::kLdsBytes, st, Sigma, Y, Na, N, ld,
                       p.gemm_tile0, p.gemm_k);
    hipLaunchKernelGGL(k_dr_bat, dim3(nb_strips, (unsigned)((Na + kBK - 1) / kBK)), dim3(kThreads), 0, st, Sigma, Phi, Y, Na,
                       N, ld, p.pitch);
    hipLaunchKernelGGL(k_dr_put_ba, dim3(nb_strips, (unsigned)((Na + 63) / 64)), dim3(kThreads), 0, st, Sigma, Y, Na, N, ld);
    hipLaunchKernelGGL(k_dr_put_ab, dim3(nb_groups, (unsigned)Na), dim3(kThreads), 0, st, Sigma, V, Na, N, ld);
}

}  // namespace ekf
