// ekf_dense64_extract.hip -- a map, or a submap, of a SOURCE handle copied into a DESTINATION handle (gfx950, wave64): the
// inverse of the join.  With keep [k] a list of distinct landmarks of the source and the index map
//   iota: 0, 1, 2 -> 0, 1, 2,   3 + 2 t + c -> 3 + 2 keep[t] + c   (c = 0, 1;  Nd = 3 + 2 k),
// Sigma_dst[i][j] takes the bits of Sigma_src[iota(i)][iota(j)] and x_dst[i] those of x_src[iota(i)], i, j < Nd.  Deleting
// rows and columns is the EKF's marginalisation, so the submap is exact; there is no arithmetic at all, a NaN keeps its
// payload and a zero its sign.  The definition is include/ekfslam.h's (ekf_dense64_extract_map); tests/dense_extract_cases.py
// holds it in numpy.  The source is read only, nothing at a destination index >= Nd is read or written.
//   k_ex_corner  the hot pass over the destination's Sigma[3:Nd, 3:Nd]: the frame and join passes' shape -- tiles of 64 rows x
//                128 columns with origins on the odd indices 3 + 64 a, 3 + 128 b, a lane per landmark of columns (a 2 x 2
//                block per lane and row landmark), eight row landmarks per wave, sixteen 16-byte loads in flight before the
//                first store, stores along the destination's rows.  The row landmarks of a wave are the same for every lane
//                and come through the scalar cache; the column of a lane is fixed before the loads are issued, so a load's
//                address is a wave-uniform row offset plus a per-lane column offset.  Per COLUMN TILE the host says (run
//                [tile], found while the list is validated) whether the tile's landmarks are a contiguous ascending run of
//                the source: then the lane's column is keep[first of the tile] + lane -- one scalar load, and a wave's sixty-
//                four 16-byte loads cover 1 KiB of one source row, the join kernel's access exactly (clone, a prefix, any list
//                of long runs).  Otherwise the lane loads its own landmark from the list and the wave's loads are sixty-four
//                16-byte pieces of one source row: the same instructions, the same result, as many cache lines as pieces.
//   k_ex_edge    a thread per landmark of the destination: its piece of the three pose rows and pose columns and its two
//                states; one more thread for the 3 x 3 corner and the pose.
//   k_ex_panels  the pending rows of the source carried, not applied: row q of both panels gathered by the same index map,
//                K_dst[q][i] = K_src[q][iota(i)], and zero from Nd up to the width the calls of that live width keep zero.
// No LDS, no atomics, no reductions: every entry is one load and one store.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense64_rot2.hpp"

namespace ekf {

namespace {

using rot2::f64x2;
using rot2::f64x2u;

constexpr int kTr = kDense64ExtractTileRows, kTc = kDense64ExtractTileCols, kThreads = kDense64ExtractThreads;
constexpr int kLr = kTr / 2, kLc = kTc / 2;      // landmarks of a tile's rows and columns
constexpr int kUnits = kLr / (kThreads / 64);    // row landmarks of a wave
constexpr int kSmall = 256;                      // threads of the two small kernels
static_assert(kLc == 64 && kUnits == 8, "a lane per landmark of columns, eight row landmarks per wave");

// ---- the pass over the destination's Sigma[3:Nd, 3:Nd] --------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_ex_corner(const double* __restrict__ SB, int ldb, double* __restrict__ SA, int lda,
                                                        int k, const int* __restrict__ keep, const int* __restrict__ run) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tc0 = kLc * blockIdx.x, tc = tc0 + lane;   // this lane's landmark of the destination's columns
    const int tr0 = kLr * blockIdx.y + kUnits * w;       // this wave's landmarks tr0 .. tr0 + kUnits - 1 of its rows
    const bool col_in = tc < k;
    // the lane's landmark of the source: a run -- the tile's first (tc0 < k always) plus the lane; else the lane's own entry.
    // The list is padded with zeros to whole tiles, and a lane or a row pair beyond k loads landmark 0 and stores nothing:
    // no load sits behind a branch.
    const int sc = run[blockIdx.x] ? keep[tc0] + lane : keep[tc];
    const double* col = SB + 3 + 2 * (size_t)(col_in ? sc : 0);
    int sr[kUnits];   // (the same addresses for every lane)
#pragma unroll
    for (int u = 0; u < kUnits; u++) sr[u] = keep[tr0 + u];

    f64x2 a[kUnits], b[kUnits];
#pragma unroll
    for (int u = 0; u < kUnits; u++) {
        const double* src = col + (size_t)(3 + 2 * sr[u]) * ldb;
        a[u] = *reinterpret_cast<const f64x2u*>(src);
        b[u] = *reinterpret_cast<const f64x2u*>(src + ldb);
    }
    double* out = SA + (size_t)(3 + 2 * tr0) * lda + 3 + 2 * tc;
#pragma unroll
    for (int u = 0; u < kUnits; u++) {
        if (tr0 + u >= k) break;   // (uniform in the wave)
        if (col_in) {
            *reinterpret_cast<f64x2u*>(out) = a[u];
            *reinterpret_cast<f64x2u*>(out + lda) = b[u];
        }
        out += 2 * (size_t)lda;
    }
}

// ---- the pose rows and columns, the 3 x 3 corner, the state -----------------------------------------------------------------
// Thread t < k: landmark t of the destination (the source's keep[t]); thread k: the pose.
__global__ __launch_bounds__(kSmall) void k_ex_edge(const double* __restrict__ SB, int ldb, const double* __restrict__ xb,
                                                    double* __restrict__ SA, int lda, double* __restrict__ xa, int k,
                                                    const int* __restrict__ keep) {
    const int t = kSmall * blockIdx.x + threadIdx.x;
    if (t > k) return;
    if (t == k) {
        double o[3][3], x[3];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            x[i] = xb[i];
#pragma unroll
            for (int j = 0; j < 3; j++) o[i][j] = SB[(size_t)i * ldb + j];
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            xa[i] = x[i];
#pragma unroll
            for (int j = 0; j < 3; j++) SA[(size_t)i * lda + j] = o[i][j];
        }
        return;
    }
    const int s = 3 + 2 * keep[t], d = 3 + 2 * t;
    double r[3][2], c[2][3], x[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        x[e] = xb[s + e];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            r[i][e] = SB[(size_t)i * ldb + s + e];
            c[e][i] = SB[(size_t)(s + e) * ldb + i];
        }
    }
#pragma unroll
    for (int e = 0; e < 2; e++) {
        xa[d + e] = x[e];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            SA[(size_t)i * lda + d + e] = r[i][e];
            SA[(size_t)(d + e) * lda + i] = c[e][i];
        }
    }
}

// ---- the pending rows ---------------------------------------------------------------------------------------------------------
// blockIdx.y: the row q; blockIdx.z: the panel (K, T); a thread per column i < upto of the destination's panels
__global__ __launch_bounds__(kSmall) void k_ex_panels(const double* __restrict__ Kb, const double* __restrict__ Tb, int ldb,
                                                      double* __restrict__ Ka, double* __restrict__ Ta, int lda, int Nd, int upto,
                                                      const int* __restrict__ keep) {
    const int i = kSmall * blockIdx.x + threadIdx.x;
    if (i >= upto) return;
    const double* src = (blockIdx.z ? Tb : Kb) + (size_t)blockIdx.y * ldb;
    double* dst = (blockIdx.z ? Ta : Ka) + (size_t)blockIdx.y * lda;
    double v = 0.0;
    if (i < 3) v = src[i];
    else if (i < Nd) v = src[3 + 2 * keep[(i - 3) >> 1] + ((i - 3) & 1)];
    dst[i] = v;
}

}  // namespace

void launch_dense64_extract(const Dense64ExtractPlan& p, double* Sigma_dst, double* state_dst, const double* Sigma_src,
                            const double* state_src, const int* ws, hipStream_t st) {
    const int *keep = ws + p.off_keep, *run = ws + p.off_run;
    if (p.k > 0)
        hipLaunchKernelGGL(k_ex_corner, dim3(p.corner_gx, p.corner_gy), dim3(kThreads), 0, st, Sigma_src, p.ld_src, Sigma_dst,
                           p.ld_dst, p.k, keep, run);
    hipLaunchKernelGGL(k_ex_edge, dim3(p.k / kSmall + 1), dim3(kSmall), 0, st, Sigma_src, p.ld_src, state_src, Sigma_dst, p.ld_dst,
                       state_dst, p.k, keep);
}

void launch_dense64_extract_panels(const Dense64ExtractPlan& p, double* K_dst, double* T_dst, const double* K_src,
                                   const double* T_src, int rows, const int* ws, hipStream_t st) {
    if (rows < 1) return;
    hipLaunchKernelGGL(k_ex_panels, dim3((p.panel_cols + kSmall - 1) / kSmall, rows, 2), dim3(kSmall), 0, st, K_src, T_src,
                       p.ld_src, K_dst, T_dst, p.ld_dst, p.Nd, p.panel_cols, ws + p.off_keep);
}

}  // namespace ekf
