// ekf_circle_fit.hpp -- device only: what rigid2d::CircleFitting::approxCirclePositions (circle_fitting.cpp:11-304) needs
// behind its clustering, written once for the two kernels that run it -- k_circles (ekf_circles.hip: one wavefront per scan,
// one LANE per cluster) and k_scan_circles (ekf_dense64_scan.hip: one workgroup per scan, one WAVE per cluster).  Here: the
// limits, the cluster record, the polar -> Cartesian prologue of one beam, the wrap merge that ends clusteringRanges(), and
// cf_fit, circleRegression() + classifyCircle() of one cluster with all of the reference's quirks.  The kernels keep their
// clustering, their way of handing clusters out, their output pass and their launcher.
// cf_fit is a template over a policy that says how the POINTS of a cluster are visited -- the sums over them (means, z_sum,
// alpha / beta / gamma of a Jacobi pair, the column norms, the inscribed-angle sum), the rows of the design matrix and their
// rotation -- and how a decision is taken.  Everything 4 x 4 (V, the sort, Y, T, Q, the symmetric eigen-solve, the
// eigenvector choice, the back-substitution, centre, radius, the thresholds) is the same code for both, fully unrolled with
// selects in place of runtime indices, so it stays in registers.  Compile with -ffp-contract=off: the order of every sum
// is the policy's and nothing else's.
#pragma once
#include "ekf_kernels.hpp"
#include "ekf_dense64_layout.hpp"

namespace ekf {

// of one scan; the numbers are the handle's (ekf_dense64_layout.hpp), which the host sizes its buffers by
constexpr int kMaxBeams = kDense64ScanMaxBeams, kMaxClusters = kDense64ScanMaxClusters;  // kMaxClusters > kMaxBeams / 7
constexpr double kClusterThres = 0.2;                                                    // :14

struct Cluster {
    int n, s0, l0, s1, l1;  // points; segment 0 (start, len), segment 1 (start, len) after a wrap merge
};

// point k of a cluster (segment 0 first, then segment 1)
__device__ __forceinline__ int cf_beam(const Cluster& c, int k) { return k < c.l0 ? c.s0 + k : c.s1 + (k - c.l0); }

// beam i of nb with the range ri: r, xs, ys
__device__ __forceinline__ void cf_polar(double ri, int i, int nb, double* r, double* xs, double* ys) {
    const double angle_resolution = 2 * kPI / (double)nb;  // circle_fitting.cpp:16
    r[i] = ri;
    if (i == 0) { xs[0] = ri * cos(0.0); ys[0] = ri * sin(0.0); }           // :25-26
    else {
        const double a = normalize_angle(i * angle_resolution);            // :44-45
        xs[i] = ri * cos(a);
        ys[i] = ri * sin(a);
    }
}

// the end of clusteringRanges() on ONE thread: the last cluster goes in front of the first when their outer ranges are
// close, then the clusters' places in the design-matrix buffer (they are disjoint: the offsets end at nb or below)
// -> the cluster count
__device__ __forceinline__ int cf_wrap_merge(Cluster* cl, int nc, const double* r, int* zoff) {
    if (nc > 0) {  // :54-70 (an empty list is UB in the reference; here: no circles)
        const double first_elem_of_first = r[cl[0].s0];
        const Cluster last = cl[nc - 1];
        const double last_elem_of_last = r[last.s0 + last.l0 - 1];
        if (fabs(first_elem_of_first - last_elem_of_last) < kClusterThres) {
            if (nc == 1) nc = 0;  // prepended to itself, then popped
            else {
                cl[0] = Cluster{last.l0 + cl[0].l0, last.s0, last.l0, cl[0].s0, cl[0].l0};
                nc--;
            }
        }
    }
    int off = 0;
    for (int c = 0; c < nc; c++) { zoff[c] = off; off += cl[c].n; }
    return nc;
}

// ---- the two policies ------------------------------------------------------------------------------------------------------
// sum(k0, k1, acc, term): acc[n] += the terms of the points k0 <= k < k1, term(k, acc) adding point k's; each(m, f): f(k)
// for every point this lane owns; at(m, k, j): where entry (k, j) of the m x 4 design matrix sits; decide(b): b as a branch
// condition.

// k_circles: the lane has the cluster to itself.  Sums in the order k = k0 .. k1 - 1, design matrix row-major.
struct LanePolicy {
    __device__ __forceinline__ int at(int, int k, int j) const { return 4 * k + j; }
    template <int N, class F> __device__ __forceinline__ void sum(int k0, int k1, double (&acc)[N], F term) const {
        for (int k = k0; k < k1; k++) term(k, acc);
    }
    template <class F> __device__ __forceinline__ void each(int m, F f) const { for (int k = 0; k < m; k++) f(k); }
    __device__ __forceinline__ bool decide(bool b) const { return b; }
};

// k_scan_circles: the wave has the cluster, point k in lane k % 64.  A sum is the lane's partial over k = lane, lane + 64, ..
// and then the fixed xor butterfly 32, 16, .., 1: its order depends on the point count alone and every lane ends with the
// same bits (a + b == b + a), so all 4 x 4 work is wave-uniform.  Design matrix column-major (column j at j m): lanes reading
// one column of consecutive points read consecutive doubles.  A decision every lane takes alike goes through the scalar
// unit -- ONLY here: under LanePolicy the lanes hold different clusters and the first lane's answer would be theirs too.
struct WavePolicy {
    int lane;
    __device__ __forceinline__ int at(int m, int k, int j) const { return j * m + k; }
    template <int N, class F> __device__ __forceinline__ void sum(int k0, int k1, double (&acc)[N], F term) const {
        for (int k = lane; k < k1; k += kWave)
            if (k >= k0) term(k, acc);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            double t[N];
#pragma unroll
            for (int n = 0; n < N; n++) t[n] = __shfl_xor(acc[n], d);
#pragma unroll
            for (int n = 0; n < N; n++) acc[n] += t[n];
        }
    }
    template <class F> __device__ __forceinline__ void each(int m, F f) const { for (int k = lane; k < m; k += kWave) f(k); }
    __device__ __forceinline__ bool decide(bool b) const { return __builtin_amdgcn_readfirstlane(b ? 1 : 0) != 0; }
};

// ---- 4 x 4, in registers -----------------------------------------------------------------------------------------------------
// (a, b) <- (c a - sn b, sn a + c b)
__device__ __forceinline__ void cf_rot(double c, double sn, double& a, double& b) {
    const double x = a, y = b;
    a = c * x - sn * y;
    b = sn * x + c * y;
}

// the Jacobi rotation that annihilates an off-diagonal entry, from zeta = (a_qq - a_pp) / (2 a_pq)
__device__ __forceinline__ void cf_jacobi(double zeta, double& c, double& sn) {
    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    c = 1.0 / sqrt(1.0 + t * t);
    sn = c * t;
}

__device__ __forceinline__ void cf_identity(double (&M)[16]) {
#pragma unroll
    for (int i = 0; i < 16; i++) M[i] = (i % 5 == 0) ? 1.0 : 0.0;
}

__device__ __forceinline__ void cf_mul4(const double (&A)[16], const double (&B)[16], double (&C)[16]) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) a += A[4 * i + k] * B[4 * k + j];
            C[4 * i + j] = a;
        }
}

// one-sided Jacobi SVD of the m x 4 matrix Z: Z <- U diag(s), s descending, V with it
template <class P>
__device__ __forceinline__ void cf_svd4(const P& pol, double* Z, int m, double (&s)[4], double (&V)[16]) {
    cf_identity(V);
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double abg[3] = {0.0, 0.0, 0.0};
                pol.sum(0, m, abg, [&](int k, double (&a)[3]) {
                    const double zp = Z[pol.at(m, k, p)], zq = Z[pol.at(m, k, q)];
                    a[0] += zp * zp; a[1] += zq * zq; a[2] += zp * zq;
                });
                const double alpha = abg[0], beta = abg[1], gamma = abg[2], lim = sqrt(alpha * beta);
                if (pol.decide(gamma == 0.0 || fabs(gamma) <= 1e-300 || fabs(gamma) <= 1e-17 * lim)) continue;
                if (fabs(gamma) > off) off = fabs(gamma) / (lim > 0 ? lim : 1.0);
                double c, sn;
                cf_jacobi((beta - alpha) / (2.0 * gamma), c, sn);
                pol.each(m, [&](int k) { cf_rot(c, sn, Z[pol.at(m, k, p)], Z[pol.at(m, k, q)]); });
#pragma unroll
                for (int k = 0; k < 4; k++) cf_rot(c, sn, V[4 * k + p], V[4 * k + q]);
            }
        if (pol.decide(off < 1e-15)) break;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double a[1] = {0.0};
        pol.sum(0, m, a, [&](int k, double (&acc)[1]) { const double z = Z[pol.at(m, k, j)]; acc[0] += z * z; });
        s[j] = sqrt(a[0]);
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i + 1; j < 4; j++) {
            const bool sw = s[j] > s[i];
            const double si = s[i], sj = s[j];
            s[i] = sw ? sj : si; s[j] = sw ? si : sj;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double vi = V[4 * k + i], vj = V[4 * k + j];
                V[4 * k + i] = sw ? vj : vi; V[4 * k + j] = sw ? vi : vj;
            }
        }
}

// cyclic Jacobi on the symmetric A: w its diagonal at the end, E the eigenvectors in columns
template <class P>
__device__ __forceinline__ void cf_eig4_sym(const P& pol, double (&A)[16], double (&w)[4], double (&E)[16]) {
    cf_identity(E);
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            diag += A[5 * i] * A[5 * i];
#pragma unroll
            for (int j = i + 1; j < 4; j++) off += A[4 * i + j] * A[4 * i + j];
        }
        if (pol.decide(off <= 1e-34 * diag || off == 0.0)) break;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[4 * p + q];
                if (pol.decide(apq == 0.0)) continue;
                double c, sn;
                cf_jacobi((A[5 * q] - A[5 * p]) / (2.0 * apq), c, sn);
#pragma unroll
                for (int k = 0; k < 4; k++) cf_rot(c, sn, A[4 * k + p], A[4 * k + q]);
#pragma unroll
                for (int k = 0; k < 4; k++) cf_rot(c, sn, A[4 * p + k], A[4 * q + k]);
#pragma unroll
                for (int k = 0; k < 4; k++) cf_rot(c, sn, E[4 * k + p], E[4 * k + q]);
            }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = A[5 * i];
}

// ---- one cluster ---------------------------------------------------------------------------------------------------------------
// circleRegression() + classifyCircle() of the cluster cc; Z: its 4 cc.n doubles of the design-matrix buffer
// -> out = x, y, r, is_circle
template <class P>
__device__ __forceinline__ void cf_fit(const P& pol, const Cluster& cc, const double* xs, const double* ys, double* Z,
                                       double (&out)[4]) {
    const int m = cc.n;
    double xy_sum[2] = {0.0, 0.0};
    pol.sum(0, m, xy_sum, [&](int k, double (&a)[2]) { const int bi = cf_beam(cc, k); a[0] += xs[bi]; a[1] += ys[bi]; });  // :112-117
    const double x_mean = xy_sum[0] / (double)m, y_mean = xy_sum[1] / (double)m;
    double z_sum[1] = {0.0};
    pol.sum(0, m, z_sum, [&](int k, double (&a)[1]) {                                              // :124-141
        const int bi = cf_beam(cc, k);
        const double x = xs[bi] - x_mean, y = ys[bi] - y_mean;
        const double zi = x * x + y * y;
        a[0] += zi;
        Z[pol.at(m, k, 0)] = zi; Z[pol.at(m, k, 1)] = x; Z[pol.at(m, k, 2)] = y; Z[pol.at(m, k, 3)] = 1.0;
    });
    const double z_mean = z_sum[0] / (double)m;
    double sv[4], V[16], A[4];
    cf_svd4(pol, Z, m, sv, V);                                                                     // :168
    if (pol.decide(sv[3] < 1e-12)) {                                                               // :171-175
#pragma unroll
        for (int k = 0; k < 4; k++) A[k] = V[4 * k + 3];
    } else {
        double Y[16], T[16], Q[16], w[4], E[16];
        // Hinv (:156-161): [0][3] = [3][0] = 0.5, [1][1] = [2][2] = 1, [3][3] = -2 z_mean
        const double Hinv[16] = {0.0, 0.0, 0.0, 0.5, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.5, 0.0, 0.0, -2.0 * z_mean};
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                double a = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) a += V[4 * i + k] * sv[k] * V[4 * j + k];
                Y[4 * i + j] = a;
            }
        cf_mul4(Y, Hinv, T);
        cf_mul4(T, Y, Q);
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = i + 1; j < 4; j++) { const double a = 0.5 * (Q[4 * i + j] + Q[4 * j + i]); Q[4 * i + j] = a; Q[4 * j + i] = a; }
        cf_eig4_sym(pol, Q, w, E);                                                                 // :184
        double best = 1000.0;                                                                      // :187-197
        double As[4] = {E[0], E[4], E[8], E[12]}, tmp[4];  // (column 0 when no eigenvalue qualifies)
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const bool take = w[e] > 0 && w[e] < best;
            best = take ? w[e] : best;
#pragma unroll
            for (int k = 0; k < 4; k++) As[k] = take ? E[4 * k + e] : As[k];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {                                                              // :211
            double a = 0.0;
#pragma unroll
            for (int i = 0; i < 4; i++) a += V[4 * i + k] * As[i];
            tmp[k] = a / sv[k];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            double a = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) a += V[4 * i + k] * tmp[k];
            A[i] = a;
        }
    }
    const double a = -A[1] / (2 * A[0]);                                                           // :220-222
    const double bq = -A[2] / (2 * A[0]);
    const double R_sqr = (A[1] * A[1] + A[2] * A[2] - 4 * A[0] * A[3]) / (4 * (A[0] * A[0]));
    const double rad = sqrt(R_sqr);
    // classifyCircle(), :234-296
    const int b1 = cf_beam(cc, 0), b2 = cf_beam(cc, m - 1);
    const double p1x = xs[b1], p1y = ys[b1], p2x = xs[b2], p2y = ys[b2];
    double sum_angle[1] = {0.0};
    pol.sum(1, m - 1, sum_angle, [&](int k, double (&acc)[1]) {
        const int bi = cf_beam(cc, k);
        const double pp1x = p1x - xs[bi], pp1y = p1y - ys[bi], pp2x = p2x - xs[bi], pp2y = p2y - ys[bi];
        const double top_part = pp1x * pp2x + pp1y * pp2y;
        const double bot_part = sqrt(pp1x * pp1x + pp1y * pp1y) * sqrt(pp2x * pp2x + pp2y * pp2y);
        acc[0] += acos(top_part / bot_part);
    });
    const double mean_angle = sum_angle[0] / (m - 2);
    const int ok = (mean_angle > 1.5708 && mean_angle < 2.3562 && rad < 0.2) ? 1 : 0;              // :264-271
    out[0] = a + x_mean; out[1] = bq + y_mean; out[2] = rad; out[3] = (double)ok;
}

}  // namespace ekf
