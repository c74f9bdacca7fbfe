// ekf_dense64_frame.hip -- the map of the dense fp64 handle re-expressed in another frame (gfx950, wave64): the congruence
// Sigma <- J Sigma J^T of the live corner for J = D + [C | 0], D = blockdiag(1, G, G, ..., G) with one 2 x 2 block G on the
// robot position and on every landmark and C an Na x 3 block on the pose columns (absent for a known rigid transform), in
// place, every entry read and written once; and the two transforms of the state that go with it.  The definition, operation
// by operation, is include/ekfslam.h's (ekf_dense64_map_congruence); tests/dense_frame_cases.py holds it in numpy.
// The states pair up as (1, 2), (3, 4), ...; index 0 stands alone.  Na is odd, so no pair straddles Na.
//   k_fr_state<MODE>  a thread per pair: the new state into a staging vector (the caller copies it over the state behind the
//                     launches, so every thread reads the OLD pose), G and -- ROBOT -- C into the terms buffer [4 + 3 Na].
//                     FIXED takes cos and sin from the host; ROBOT takes them on the device from the handle's own heading.
//   k_fr_panels<C>    a thread per pair: the three OLD pose rows (along rows) and the three OLD pose columns (the only walk
//                     down a column, 3 Na entries) go into the workspace as [3][ld] each; with C also the nine panel rows
//                     A (3) | C^T (3) | (D Sigma_c)^T (3) in the handle's [k][ld] layout: rows 0 .. 5 are the 6-row panel of
//                     a tile's columns, rows 3 .. 8 the 6-row panel of its rows.  Reads Sigma, writes none of it.
//   k_fr_pose<C>      a thread per pair: the NEW pose rows and pose columns (and the 3 x 3 corner) from that snapshot alone.
//   k_fr_update<C>    the pass over Sigma[3:Na, 3:Na]: tiles of 64 rows x 128 columns whose origins sit on the odd indices
//                     3 + 64 a, 3 + 128 b, so no 2 x 2 block straddles two workgroups.  A lane owns one pair of columns, a
//                     wave eight pairs of rows: sixteen 16-byte loads along rows are issued before the first is used (64 KiB
//                     in flight per workgroup), the block is rotated from both sides in registers, the six fused steps of the
//                     rank-6 term follow, and the block goes back where it came from -- no staging copy of Sigma, no LDS.
//                     The panel of the lane's columns sits in 24 vector registers for the life of the workgroup, the panel of
//                     a row pair is the same for the whole wave and comes through the scalar cache.  Every load and store is
//                     masked by row < Na and column < Na (a pair is inside or outside as a whole), whatever N and ld are:
//                     the odd origins never line up with ld, so there is no unmasked variant for a handle without a tail.
// No atomics, no reductions: an entry's bits depend on its own 2 x 2 block, G and the panel entries of its row and column.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense64_rot2.hpp"

namespace ekf {

namespace {

constexpr int kTr = kDense64FrameTileRows, kTc = kDense64FrameTileCols, kThreads = kDense64FrameThreads;
constexpr int kUnits = kTr / 2 / (kThreads / 64);   // row pairs of a wave
constexpr int kSmall = 256;                         // threads of the three small kernels
static_assert(kTc == 2 * 64 && kUnits == 8, "a lane per pair of columns, eight pairs of rows per wave");

using namespace rot2;   // f64x2, f64x2u, one_sided, both_sided: the rotation of a 2 x 2 block (ekf_dense64_rot2.hpp)

// ---- the state and the terms ----------------------------------------------------------------------------------------------
// terms: G [4] | C [Na][3].  xs [Na]: the new state.  Thread p: index 0 (p = 0) or the pair (2 p - 1, 2 p).
template <int MODE>
__global__ __launch_bounds__(kSmall) void k_fr_state(const double* __restrict__ x, int Na, double* __restrict__ terms,
                                                     double* __restrict__ xs, double dtheta, double c, double s, double tx,
                                                     double ty) {
    const int p = kSmall * blockIdx.x + threadIdx.x;
    if (2 * p >= Na) return;
    double* Cm = terms + 4;
    if (MODE == kDense64FrameFixed) {
        if (p == 0) {
            xs[0] = x[0] + dtheta;
            terms[0] = c, terms[1] = -s, terms[2] = s, terms[3] = c;
            return;
        }
        const int j = 2 * p - 1;
        const double X = x[j], Y = x[j + 1];
        xs[j] = fma(-s, Y, c * X) + tx;
        xs[j + 1] = fma(c, Y, s * X) + ty;
    } else {   // M = R(-theta) = [c s; -s c], M' = dM/dtheta = [-s c; -c -s], so M' v = ((M v).y, -(M v).x)
        const double th = x[0], px = x[1], py = x[2];
        c = cos(th), s = sin(th);
        if (p == 0) {
            xs[0] = -th;
            terms[0] = c, terms[1] = s, terms[2] = -s, terms[3] = c;
            Cm[0] = -2.0, Cm[1] = 0.0, Cm[2] = 0.0;
            return;
        }
        const int j = 2 * p - 1;
        if (p == 1) {   // p' = -M p;  rows [-M' p | -2 M]
            const double mx = fma(s, py, c * px), my = fma(c, py, -s * px);
            xs[1] = -mx, xs[2] = -my;
            Cm[3] = -my, Cm[4] = -2.0 * c, Cm[5] = -2.0 * s;
            Cm[6] = mx, Cm[7] = 2.0 * s, Cm[8] = -2.0 * c;
            return;
        }
        const double dx = x[j] - px, dy = x[j + 1] - py;   // l' = M (l - p);  rows [M' (l - p) | -M]
        const double mx = fma(s, dy, c * dx), my = fma(c, dy, -s * dx);
        xs[j] = mx, xs[j + 1] = my;
        double* r = Cm + 3 * (size_t)j;
        r[0] = my, r[1] = -c, r[2] = -s;
        r[3] = -mx, r[4] = s, r[5] = -c;
    }
}

// ---- the snapshot of the pose rows and columns, and the panels --------------------------------------------------------------
// rows [3][ld]: rows[k][j] = Sigma[k][j];  cols [3][ld]: cols[k][j] = Sigma[j][k];  pan [9][ld]: A | C^T | Bc^T (HAS_C only)
template <bool HAS_C>
__global__ __launch_bounds__(kSmall) void k_fr_panels(const double* __restrict__ S, int ld, int Na,
                                                      const double* __restrict__ terms, double* __restrict__ rows,
                                                      double* __restrict__ cols, double* __restrict__ pan) {
    const int p = kSmall * blockIdx.x + threadIdx.x;
    if (2 * p >= Na) return;
    const double G[4] = {terms[0], terms[1], terms[2], terms[3]};
    const double* Cm = terms + 4;
    const int j = p == 0 ? 0 : 2 * p - 1, n = p == 0 ? 1 : 2;   // this thread's indices j .. j + n - 1
    double r[3][2], cl[2][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int e = 0; e < 2; e++) {
            r[k][e] = e < n ? S[(size_t)k * ld + j + e] : 0.0;
            cl[e][k] = e < n ? S[(size_t)(j + e) * ld + k] : 0.0;
        }
#pragma unroll
    for (int k = 0; k < 3; k++)
        for (int e = 0; e < n; e++) {
            rows[(size_t)k * ld + j + e] = r[k][e];
            cols[(size_t)k * ld + j + e] = cl[e][k];
        }
    if (!HAS_C) return;
    double pp[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int l = 0; l < 3; l++) pp[k][l] = S[(size_t)k * ld + l];
    for (int e = 0; e < n; e++) {
        const double* cj = Cm + 3 * (size_t)(j + e);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            // A = Sigma_p D^T + Sigma_pp C^T, the second term by fused steps in ascending index;  Bc = D Sigma_c
            double a = p == 0 ? r[k][0] : one_sided(G[2 * e], G[2 * e + 1], r[k][0], r[k][1]);
            a = fma(pp[k][0], cj[0], a);
            a = fma(pp[k][1], cj[1], a);
            a = fma(pp[k][2], cj[2], a);
            pan[(size_t)k * ld + j + e] = a;
            pan[(size_t)(3 + k) * ld + j + e] = cj[k];
            pan[(size_t)(6 + k) * ld + j + e] = p == 0 ? cl[0][k] : one_sided(G[2 * e], G[2 * e + 1], cl[0][k], cl[1][k]);
        }
    }
}

// P[i][j] + sum_k C[i][k] A[k][j] + sum_k Bc[i][k] C[j][k]: six fused steps, the C A terms first, k ascending
template <bool HAS_C>
__device__ __forceinline__ double rank6(double acc, const double* __restrict__ pan, int ld, int i, int j) {
    if (!HAS_C) return acc;
#pragma unroll
    for (int k = 0; k < 3; k++) acc = fma(pan[(size_t)(3 + k) * ld + i], pan[(size_t)k * ld + j], acc);
#pragma unroll
    for (int k = 0; k < 3; k++) acc = fma(pan[(size_t)(6 + k) * ld + i], pan[(size_t)(3 + k) * ld + j], acc);
    return acc;
}

// ---- the new pose rows and columns, from the snapshot alone -------------------------------------------------------------------
template <bool HAS_C>
__global__ __launch_bounds__(kSmall) void k_fr_pose(double* __restrict__ S, int ld, int Na, const double* __restrict__ terms,
                                                    const double* __restrict__ rows, const double* __restrict__ cols,
                                                    const double* __restrict__ pan) {
    const int p = kSmall * blockIdx.x + threadIdx.x;
    if (2 * p >= Na || p == 1) return;   // (thread 0 takes the whole 3 x 3 corner)
    const double G[4] = {terms[0], terms[1], terms[2], terms[3]};
    if (p == 0) {   // the corner: index 0 alone, the pair (1, 2); the old entries are rows[i][j], i, j < 3
        double o[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) o[i][j] = rows[(size_t)i * ld + j];
        double P[3][3];
        P[0][0] = o[0][0];
        P[0][1] = one_sided(G[0], G[1], o[0][1], o[0][2]);
        P[0][2] = one_sided(G[2], G[3], o[0][1], o[0][2]);
        P[1][0] = one_sided(G[0], G[1], o[1][0], o[2][0]);
        P[2][0] = one_sided(G[2], G[3], o[1][0], o[2][0]);
        f64x2 za, zb;
        both_sided(G, f64x2{o[1][1], o[1][2]}, f64x2{o[2][1], o[2][2]}, &za, &zb);
        P[1][1] = za[0], P[1][2] = za[1], P[2][1] = zb[0], P[2][2] = zb[1];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) S[(size_t)i * ld + j] = rank6<HAS_C>(P[i][j], pan, ld, i, j);
        return;
    }
    const int j = 2 * p - 1;   // >= 3
    {   // the pose rows at the columns (j, j + 1)
        const f64x2 r0 = {rows[j], rows[j + 1]};
        const f64x2 r1 = {rows[(size_t)ld + j], rows[(size_t)ld + j + 1]};
        const f64x2 r2 = {rows[(size_t)2 * ld + j], rows[(size_t)2 * ld + j + 1]};
        f64x2 z[3];
        z[0] = f64x2{one_sided(G[0], G[1], r0[0], r0[1]), one_sided(G[2], G[3], r0[0], r0[1])};
        both_sided(G, r1, r2, &z[1], &z[2]);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int e = 0; e < 2; e++) S[(size_t)i * ld + j + e] = rank6<HAS_C>(z[i][e], pan, ld, i, j + e);
    }
    {   // the pose columns at the rows (j, j + 1): Sigma[j + e][k] = cols[k][j + e]
        const f64x2 c0 = {cols[j], cols[j + 1]};
        const f64x2 a = {cols[(size_t)ld + j], cols[(size_t)2 * ld + j]};           // row j, columns 1, 2
        const f64x2 b = {cols[(size_t)ld + j + 1], cols[(size_t)2 * ld + j + 1]};   // row j + 1
        f64x2 za, zb;
        both_sided(G, a, b, &za, &zb);
        const double top[3] = {one_sided(G[0], G[1], c0[0], c0[1]), za[0], za[1]};
        const double bot[3] = {one_sided(G[2], G[3], c0[0], c0[1]), zb[0], zb[1]};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            S[(size_t)j * ld + k] = rank6<HAS_C>(top[k], pan, ld, j, k);
            S[(size_t)(j + 1) * ld + k] = rank6<HAS_C>(bot[k], pan, ld, j + 1, k);
        }
    }
}

// ---- the pass over Sigma[3:Na, 3:Na] --------------------------------------------------------------------------------------------
template <bool HAS_C>
__global__ __launch_bounds__(kThreads) void k_fr_update(double* __restrict__ S, int ld, int Na, const double* __restrict__ terms,
                                                        const double* __restrict__ pan) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = 3 + kTc * blockIdx.x + 2 * lane;         // this lane's columns j, j + 1
    const int i0 = 3 + kTr * blockIdx.y + 2 * kUnits * w;  // this wave's rows i0 .. i0 + 2 kUnits - 1
    const bool col_in = j < Na;                            // (Na and j are odd: j < Na means j + 1 < Na)

    f64x2 a[kUnits], b[kUnits];
#pragma unroll
    for (int u = 0; u < kUnits; u++) {
        const int i = i0 + 2 * u;
        const bool in = col_in && i < Na;
        const double* src = S + (size_t)i * ld + j;
        a[u] = in ? *reinterpret_cast<const f64x2u*>(src) : f64x2{0.0, 0.0};
        b[u] = in ? *reinterpret_cast<const f64x2u*>(src + ld) : f64x2{0.0, 0.0};
    }
    const double G[4] = {terms[0], terms[1], terms[2], terms[3]};
    f64x2 qa[3], qc[3];   // the panel of this lane's columns: A[k][j], C[j][k]
    if (HAS_C) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            qa[k] = col_in ? *reinterpret_cast<const f64x2u*>(pan + (size_t)k * ld + j) : f64x2{0.0, 0.0};
            qc[k] = col_in ? *reinterpret_cast<const f64x2u*>(pan + (size_t)(3 + k) * ld + j) : f64x2{0.0, 0.0};
        }
    }
#pragma unroll
    for (int u = 0; u < kUnits; u++) {
        const int i = i0 + 2 * u;
        if (i >= Na) break;   // (uniform in the wave)
        f64x2 za, zb;
        both_sided(G, a[u], b[u], &za, &zb);
        if (HAS_C) {   // the panel of the row pair: C[i][k], Bc[i][k] -- the same addresses for every lane
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double c0 = pan[(size_t)(3 + k) * ld + i], c1 = pan[(size_t)(3 + k) * ld + i + 1];
                za = f64x2{fma(c0, qa[k][0], za[0]), fma(c0, qa[k][1], za[1])};
                zb = f64x2{fma(c1, qa[k][0], zb[0]), fma(c1, qa[k][1], zb[1])};
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double b0 = pan[(size_t)(6 + k) * ld + i], b1 = pan[(size_t)(6 + k) * ld + i + 1];
                za = f64x2{fma(b0, qc[k][0], za[0]), fma(b0, qc[k][1], za[1])};
                zb = f64x2{fma(b1, qc[k][0], zb[0]), fma(b1, qc[k][1], zb[1])};
            }
        }
        if (col_in) {
            double* dst = S + (size_t)i * ld + j;
            *reinterpret_cast<f64x2u*>(dst) = za;
            *reinterpret_cast<f64x2u*>(dst + ld) = zb;
        }
    }
}

}  // namespace

Dense64FramePlan dense64_frame_plan(int Na, int ld) {
    Dense64FramePlan p{};
    p.Na = Na;
    p.ld = ld;
    p.pairs = (Na + 1) / 2;
    p.off_terms = 0;
    p.off_state = 4 + 3 * (size_t)ld;
    p.off_rows = p.off_state + ld;
    p.off_cols = p.off_rows + 3 * (size_t)ld;
    p.off_panels = p.off_cols + 3 * (size_t)ld;
    p.doubles = p.off_panels + 9 * (size_t)ld;
    return p;
}

void launch_dense64_frame_state(const Dense64FramePlan& p, int mode, const double* state, double* ws, double dtheta, double c,
                                double s, double tx, double ty, hipStream_t st) {
    const dim3 grid((p.pairs + kSmall - 1) / kSmall), block(kSmall);
    if (mode == kDense64FrameFixed)
        hipLaunchKernelGGL(k_fr_state<kDense64FrameFixed>, grid, block, 0, st, state, p.Na, ws + p.off_terms,
                           ws + p.off_state, dtheta, c, s, tx, ty);
    else
        hipLaunchKernelGGL(k_fr_state<kDense64FrameRobot>, grid, block, 0, st, state, p.Na, ws + p.off_terms,
                           ws + p.off_state, 0.0, 0.0, 0.0, 0.0, 0.0);
}

namespace {
template <bool HAS_C>
void launch_congruence(const Dense64FramePlan& p, double* Sigma, double* ws, hipStream_t st) {
    const dim3 grid((p.pairs + kSmall - 1) / kSmall), block(kSmall);
    const double* terms = ws + p.off_terms;
    double *rows = ws + p.off_rows, *cols = ws + p.off_cols, *pan = ws + p.off_panels;
    hipLaunchKernelGGL(k_fr_panels<HAS_C>, grid, block, 0, st, Sigma, p.ld, p.Na, terms, rows, cols, pan);
    if (p.Na > 3)
        hipLaunchKernelGGL(k_fr_update<HAS_C>, dim3((p.Na - 3 + kTc - 1) / kTc, (p.Na - 3 + kTr - 1) / kTr), dim3(kThreads), 0, st,
                           Sigma, p.ld, p.Na, terms, pan);
    hipLaunchKernelGGL(k_fr_pose<HAS_C>, grid, block, 0, st, Sigma, p.ld, p.Na, terms, rows, cols, pan);
}
}  // namespace

void launch_dense64_frame_congruence(const Dense64FramePlan& p, double* Sigma, double* ws, bool has_C, hipStream_t st) {
    if (has_C) launch_congruence<true>(p, Sigma, ws, st);
    else launch_congruence<false>(p, Sigma, ws, st);
}

}  // namespace ekf
