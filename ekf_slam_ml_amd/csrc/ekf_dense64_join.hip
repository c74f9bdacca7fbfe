// ekf_dense64_join.hip -- map joining on the dense fp64 handles (gfx950, wave64): the map B of a SOURCE handle, built in the
// frame of the destination's robot pose and independent of it, is appended to the map A of the DESTINATION.  With
// D = blockdiag(1, G, ..., G) over the source's pairs (1, 2), (3, 4), ... and E (Nb x 3) on the destination's pose,
//   Y = D Sigma_B D^T + E Sigma_pp E^T,   X_rows = E P,   X_cols = Pc E^T
// (P, Pc, Sigma_pp: the destination's three pose rows, pose columns and 3 x 3 corner ON ENTRY), placed by the index map
// iota: 0, 1, 2 -> 0, 1, 2 and 3 + t -> Na + t.  The destination's Sigma[3:Na, 3:Na] is neither read nor written, the source
// is read only.  The definition, operation by operation, is include/ekfslam.h's (ekf_dense64_join_congruence);
// tests/dense_join_cases.py holds it in numpy.  Na and Nb are odd, so no pair straddles Na, Nb or Na + Nb - 3.
//   k_jn_state   a thread per pair of the source: cos and sin of the destination's own heading on the device, G and E into
//                the terms buffer [4 + 3 Nb], the composed pose into a staging slot (the caller copies it over the pose
//                behind the launches, so every thread reads the OLD pose), B's landmarks in A's frame into x[Na ...].
//   k_jn_snap    a thread per pair: the destination's three OLD pose rows (along rows) and three OLD pose columns (the only
//                walk down a column of the destination, 3 Na entries) into the workspace as [3][ld] each, and W = E Sigma_pp
//                [Nb][3].  Reads Sigma, writes none of it.
//   k_jn_corner  the hot pass over the source's Sigma[3:Nb, 3:Nb]: the frame pass's shape (ekf_dense64_frame.hip) with two
//                matrices -- tiles of 64 rows x 128 columns with origins on the odd indices 3 + 64 a, 3 + 128 b, a lane per
//                pair of columns, eight pairs of rows per wave, sixteen 16-byte loads along the source's rows in flight before
//                the first is used, the block rotated from both sides in registers, three fused steps of W E^T, and the block
//                stored at the destination's (Na - 3 + i, Na - 3 + j) with the destination's ld.  E of the lane's columns
//                sits in six vector registers, W of a row pair is the same for the whole wave and comes through the scalar
//                cache.  Out of place: no hazard, no LDS.  Masked by row < Nb and column < Nb, whatever N and ld are.
//   k_jn_cross   the two rectangles X_rows[3:, 3:Na] -> Sigma'[Na ..][3:Na] and X_cols[3:Na, 3:] -> Sigma'[3:Na][Na ..]: rank-3
//                products of the snapshot and E, streaming stores along rows, a lane per pair of columns.
//   k_jn_pose    a thread per pair of the joined map: the three NEW pose rows and columns over [0, Na + Nb - 3) and the 3 x 3
//                corner, from the snapshot, W, E and the source's own pose rows and columns.
// No atomics, no reductions: an entry's bits depend on its own 2 x 2 block of the source (or its three snapshot entries), G
// and the rows of E and W of its row and column.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense64_rot2.hpp"

namespace ekf {

namespace {

using namespace rot2;   // f64x2, f64x2u, one_sided, both_sided

constexpr int kTr = kDense64JoinTileRows, kTc = kDense64JoinTileCols, kThreads = kDense64JoinThreads;
constexpr int kUnits = kTr / 2 / (kThreads / 64);   // row pairs of a wave
constexpr int kSmall = 256;                         // threads of the three small kernels
constexpr int kXr = kDense64JoinCrossRows, kXc = kDense64JoinCrossCols;
static_assert(kTc == 2 * 64 && kUnits == 8, "a lane per pair of columns, eight pairs of rows per wave");
static_assert(kXc == 2 * kThreads, "a lane per pair of columns of a rectangle");

// e . q = fma(e2, q2, fma(e1, q1, fl(e0 q0))): a row of E against a column of P (or a row of Pc against a row of E)
__device__ __forceinline__ double dot3(double e0, double e1, double e2, double q0, double q1, double q2) {
    return fma(e2, q2, fma(e1, q1, e0 * q0));
}
// acc + w . e by three fused steps in ascending index
__device__ __forceinline__ double rank3(double acc, const double* __restrict__ w, const double* __restrict__ e) {
    return fma(w[2], e[2], fma(w[1], e[1], fma(w[0], e[0], acc)));
}

// ---- the state and the terms ----------------------------------------------------------------------------------------------
// terms: G [4] | E [Nb][3].  Thread p: index 0 of the source (p = 0) or its pair (2 p - 1, 2 p).  xa is read at 0, 1, 2 and
// written from Na on; pose [3] is the staging slot.
__global__ __launch_bounds__(kSmall) void k_jn_state(double* __restrict__ xa, int Na, const double* __restrict__ xb, int Nb,
                                                     double* __restrict__ terms, double* __restrict__ pose) {
    const int p = kSmall * blockIdx.x + threadIdx.x;
    if (2 * p >= Nb) return;
    const double th = xa[0], px = xa[1], py = xa[2];
    const double c = cos(th), s = sin(th);
    double* E = terms + 4;
    if (p == 0) {
        pose[0] = th + xb[0];
        terms[0] = c, terms[1] = -s, terms[2] = s, terms[3] = c;
        E[0] = 1.0, E[1] = 0.0, E[2] = 0.0;
        return;
    }
    const int j = 2 * p - 1;
    const double X = xb[j], Y = xb[j + 1];
    const double mx = fma(-s, Y, c * X), my = fma(c, Y, s * X);   // M q;  M' q = (-(M q).y, (M q).x)
    double* out = p == 1 ? pose + 1 : xa + Na + (j - 3);
    out[0] = mx + px, out[1] = my + py;
    double* r = E + 3 * (size_t)j;
    r[0] = -my, r[1] = 1.0, r[2] = 0.0;
    r[3] = mx, r[4] = 0.0, r[5] = 1.0;
}

// ---- the snapshot of the destination's pose rows and columns, and W ---------------------------------------------------------
// rows [3][ld]: rows[k][j] = Sigma[k][j];  cols [3][ld]: cols[k][j] = Sigma[j][k], j < Na;  W [Nb][3] = E Sigma_pp
__global__ __launch_bounds__(kSmall) void k_jn_snap(const double* __restrict__ S, int ld, int Na, int Nb,
                                                    const double* __restrict__ terms, double* __restrict__ rows,
                                                    double* __restrict__ cols, double* __restrict__ W) {
    const int p = kSmall * blockIdx.x + threadIdx.x;
    const int j = p == 0 ? 0 : 2 * p - 1, n = p == 0 ? 1 : 2;   // this thread's indices j .. j + n - 1
    if (j < Na) {
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
    }
    if (j < Nb) {
        const double* E = terms + 4;
        double pp[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int l = 0; l < 3; l++) pp[k][l] = S[(size_t)k * ld + l];
        for (int e = 0; e < n; e++) {
            const double* ek = E + 3 * (size_t)(j + e);
#pragma unroll
            for (int l = 0; l < 3; l++) W[3 * (size_t)(j + e) + l] = dot3(ek[0], ek[1], ek[2], pp[0][l], pp[1][l], pp[2][l]);
        }
    }
}

// ---- the pass over the source's Sigma[3:Nb, 3:Nb] -----------------------------------------------------------------------------
// shift = Na - 3 (even): the source's (i, j) goes to the destination's (shift + i, shift + j)
__global__ __launch_bounds__(kThreads) void k_jn_corner(const double* __restrict__ SB, int ldb, int Nb, double* __restrict__ SA,
                                                        int lda, int shift, const double* __restrict__ terms,
                                                        const double* __restrict__ W) {
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = 3 + kTc * blockIdx.x + 2 * lane;         // this lane's columns j, j + 1 of the source
    const int i0 = 3 + kTr * blockIdx.y + 2 * kUnits * w;  // this wave's rows i0 .. i0 + 2 kUnits - 1
    const bool col_in = j < Nb;                            // (Nb and j are odd: j < Nb means j + 1 < Nb)

    f64x2 a[kUnits], b[kUnits];
#pragma unroll
    for (int u = 0; u < kUnits; u++) {
        const int i = i0 + 2 * u;
        const bool in = col_in && i < Nb;
        const double* src = SB + (size_t)i * ldb + j;
        a[u] = in ? *reinterpret_cast<const f64x2u*>(src) : f64x2{0.0, 0.0};
        b[u] = in ? *reinterpret_cast<const f64x2u*>(src + ldb) : f64x2{0.0, 0.0};
    }
    const double G[4] = {terms[0], terms[1], terms[2], terms[3]};
    const double* E = terms + 4;
    double e0[3], e1[3];   // E of this lane's columns
#pragma unroll
    for (int l = 0; l < 3; l++) {
        e0[l] = col_in ? E[3 * (size_t)j + l] : 0.0;
        e1[l] = col_in ? E[3 * (size_t)j + 3 + l] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kUnits; u++) {
        const int i = i0 + 2 * u;
        if (i >= Nb) break;   // (uniform in the wave)
        f64x2 za, zb;
        both_sided(G, a[u], b[u], &za, &zb);
        const double* wi = W + 3 * (size_t)i;   // W of the row pair -- the same addresses for every lane
#pragma unroll
        for (int l = 0; l < 3; l++) {
            const double w0 = wi[l], w1 = wi[3 + l];
            za = f64x2{fma(w0, e0[l], za[0]), fma(w0, e1[l], za[1])};
            zb = f64x2{fma(w1, e0[l], zb[0]), fma(w1, e1[l], zb[1])};
        }
        if (col_in) {
            double* dst = SA + (size_t)(shift + i) * lda + shift + j;
            *reinterpret_cast<f64x2u*>(dst) = za;
            *reinterpret_cast<f64x2u*>(dst + lda) = zb;
        }
    }
}

// ---- the two rectangles ---------------------------------------------------------------------------------------------------------
// ROWS:  Sigma'[Na + t][j] = E[3 + t] . P[:, j],   t < Nb - 3, 3 <= j < Na: the rectangle has Nb - 3 rows and Na - 3 columns
// !ROWS: Sigma'[i][Na + t] = Pc[i] . E[3 + t],     3 <= i < Na, t < Nb - 3: Na - 3 rows and Nb - 3 columns
// A workgroup writes kXr rows of kXc columns; a lane owns one pair of columns (both origins are odd: whole pairs).
template <bool ROWS>
__global__ __launch_bounds__(kThreads) void k_jn_cross(double* __restrict__ S, int ld, int Na, int Nb,
                                                       const double* __restrict__ terms, const double* __restrict__ rows,
                                                       const double* __restrict__ cols) {
    const double* E = terms + 4;
    const int nr = ROWS ? Nb - 3 : Na - 3, nc = ROWS ? Na - 3 : Nb - 3;
    const int c = kXc * blockIdx.x + 2 * threadIdx.x;   // this lane's columns c, c + 1 of the rectangle
    if (c >= nc) return;                                // (nc is even: c < nc means c + 1 < nc)
    double q[2][3];   // of the lane's columns: P[:, 3 + c + e] (ROWS) or E[3 + c + e] (!ROWS)
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
        for (int l = 0; l < 3; l++) q[e][l] = ROWS ? rows[(size_t)l * ld + 3 + c + e] : E[3 * (size_t)(3 + c + e) + l];
    const int r0 = kXr * blockIdx.y;
#pragma unroll
    for (int u = 0; u < kXr; u++) {
        const int r = r0 + u;
        if (r >= nr) break;   // (uniform in the workgroup)
        double p[3];          // of the row: E[3 + r] (ROWS) or Pc[3 + r] (!ROWS) -- the same addresses for every lane
#pragma unroll
        for (int l = 0; l < 3; l++) p[l] = ROWS ? E[3 * (size_t)(3 + r) + l] : cols[(size_t)l * ld + 3 + r];
        const f64x2 v = {dot3(p[0], p[1], p[2], q[0][0], q[0][1], q[0][2]), dot3(p[0], p[1], p[2], q[1][0], q[1][1], q[1][2])};
        double* dst = ROWS ? S + (size_t)(Na + r) * ld + 3 + c : S + (size_t)(3 + r) * ld + Na + c;
        *reinterpret_cast<f64x2u*>(dst) = v;
    }
}

// ---- the new pose rows and columns ------------------------------------------------------------------------------------------------
// Thread p: the joined map's index 0 (p = 0, which takes the whole 3 x 3 corner) or its pair (2 p - 1, 2 p).  Below Na the
// pair is A's: the cross terms of the pose rows of E.  From Na on it is B's pair sj = j - Na + 3: Y of the source's pose rows
// and columns.
__global__ __launch_bounds__(kSmall) void k_jn_pose(double* __restrict__ SA, int lda, int Na, const double* __restrict__ SB,
                                                    int ldb, int Nb, const double* __restrict__ terms,
                                                    const double* __restrict__ rows, const double* __restrict__ cols,
                                                    const double* __restrict__ W) {
    const int p = kSmall * blockIdx.x + threadIdx.x;
    if (2 * p >= Na + Nb - 3 || p == 1) return;
    const double G[4] = {terms[0], terms[1], terms[2], terms[3]};
    const double* E = terms + 4;
    if (p == 0) {   // the corner: Z of the source's 3 x 3 corner (index 0 alone, the pair (1, 2)), then W E^T
        double o[3][3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) o[i][j] = SB[(size_t)i * ldb + j];
        double Z[3][3];
        Z[0][0] = o[0][0];
        Z[0][1] = one_sided(G[0], G[1], o[0][1], o[0][2]);
        Z[0][2] = one_sided(G[2], G[3], o[0][1], o[0][2]);
        Z[1][0] = one_sided(G[0], G[1], o[1][0], o[2][0]);
        Z[2][0] = one_sided(G[2], G[3], o[1][0], o[2][0]);
        f64x2 za, zb;
        both_sided(G, f64x2{o[1][1], o[1][2]}, f64x2{o[2][1], o[2][2]}, &za, &zb);
        Z[1][1] = za[0], Z[1][2] = za[1], Z[2][1] = zb[0], Z[2][2] = zb[1];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) SA[(size_t)i * lda + j] = rank3(Z[i][j], W + 3 * i, E + 3 * j);
        return;
    }
    const int j = 2 * p - 1;   // >= 3
    if (j < Na) {
#pragma unroll
        for (int k = 0; k < 3; k++)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                // X_rows[k][j + e] = E[k] . P[:, j + e];  X_cols[j + e][k] = Pc[j + e] . E[k]
                SA[(size_t)k * lda + j + e] = dot3(E[3 * k], E[3 * k + 1], E[3 * k + 2], rows[j + e], rows[(size_t)lda + j + e],
                                                   rows[(size_t)2 * lda + j + e]);
                SA[(size_t)(j + e) * lda + k] = dot3(cols[j + e], cols[(size_t)lda + j + e], cols[(size_t)2 * lda + j + e], E[3 * k],
                                                     E[3 * k + 1], E[3 * k + 2]);
            }
        return;
    }
    const int sj = j - Na + 3;   // the source's pair (sj, sj + 1), sj >= 3
    {   // the pose rows at the columns (j, j + 1)
        const f64x2 r0 = {SB[sj], SB[sj + 1]};
        const f64x2 r1 = {SB[(size_t)ldb + sj], SB[(size_t)ldb + sj + 1]};
        const f64x2 r2 = {SB[(size_t)2 * ldb + sj], SB[(size_t)2 * ldb + sj + 1]};
        f64x2 z[3];
        z[0] = f64x2{one_sided(G[0], G[1], r0[0], r0[1]), one_sided(G[2], G[3], r0[0], r0[1])};
        both_sided(G, r1, r2, &z[1], &z[2]);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int e = 0; e < 2; e++) SA[(size_t)i * lda + j + e] = rank3(z[i][e], W + 3 * i, E + 3 * (size_t)(sj + e));
    }
    {   // the pose columns at the rows (j, j + 1)
        const double* top_row = SB + (size_t)sj * ldb;
        const double* bot_row = top_row + ldb;
        f64x2 za, zb;
        both_sided(G, f64x2{top_row[1], top_row[2]}, f64x2{bot_row[1], bot_row[2]}, &za, &zb);
        const double top[3] = {one_sided(G[0], G[1], top_row[0], bot_row[0]), za[0], za[1]};
        const double bot[3] = {one_sided(G[2], G[3], top_row[0], bot_row[0]), zb[0], zb[1]};
#pragma unroll
        for (int k = 0; k < 3; k++) {
            SA[(size_t)j * lda + k] = rank3(top[k], W + 3 * (size_t)sj, E + 3 * k);
            SA[(size_t)(j + 1) * lda + k] = rank3(bot[k], W + 3 * (size_t)(sj + 1), E + 3 * k);
        }
    }
}

}  // namespace

void launch_dense64_join_state(const Dense64JoinPlan& p, double* state_dst, const double* state_src, double* ws, hipStream_t st) {
    hipLaunchKernelGGL(k_jn_state, dim3((p.pairs_src + kSmall - 1) / kSmall), dim3(kSmall), 0, st, state_dst, p.Na, state_src,
                       p.Nb, ws + p.off_terms, ws + p.off_pose);
}

void launch_dense64_join_congruence(const Dense64JoinPlan& p, double* Sigma_dst, const double* Sigma_src, double* ws,
                                    hipStream_t st) {
    const double* terms = ws + p.off_terms;
    double *rows = ws + p.off_rows, *cols = ws + p.off_cols, *W = ws + p.off_W;
    const int lda = p.ld_dst, ldb = p.ld_src;
    const int snap = p.pairs_dst > p.pairs_src ? p.pairs_dst : p.pairs_src;
    hipLaunchKernelGGL(k_jn_snap, dim3((snap + kSmall - 1) / kSmall), dim3(kSmall), 0, st, Sigma_dst, lda, p.Na, p.Nb, terms, rows,
                       cols, W);
    if (p.Nb > 3) {
        hipLaunchKernelGGL(k_jn_corner, dim3(p.corner_gx, p.corner_gy), dim3(kThreads), 0, st, Sigma_src, ldb, p.Nb, Sigma_dst,
                           lda, p.Na - 3, terms, W);
        if (p.Na > 3) {
            hipLaunchKernelGGL(k_jn_cross<true>, dim3(p.rows_gx, p.rows_gy), dim3(kThreads), 0, st, Sigma_dst, lda, p.Na, p.Nb,
                               terms, rows, cols);
            hipLaunchKernelGGL(k_jn_cross<false>, dim3(p.cols_gx, p.cols_gy), dim3(kThreads), 0, st, Sigma_dst, lda, p.Na, p.Nb,
                               terms, rows, cols);
        }
    }
    hipLaunchKernelGGL(k_jn_pose, dim3((p.pairs_j + kSmall - 1) / kSmall), dim3(kSmall), 0, st, Sigma_dst, lda, p.Na, Sigma_src,
                       ldb, p.Nb, terms, rows, cols, W);
}

}  // namespace ekf
