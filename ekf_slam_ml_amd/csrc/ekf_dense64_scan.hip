// ekf_dense64_scan.hip -- rigid2d::CircleFitting::approxCirclePositions (circle_fitting.cpp:11-304) for ONE laser scan, shaped
// for latency: the input of the dense fp64 handle's scan calls (ekf_dense64_fit_scan, ekf_dense64_associate_scan).  It does
// what k_circles (ekf_circles.hip, one wavefront per scan, one LANE per cluster, built for thousands of scans) does, quirk
// for quirk, with the work of a single scan spread over one workgroup of four waves:
//   clustering   every beam computes its own boundary flag from r[i], r[i - 1]; a wave's 64 flags are one ballot word; a
//                cluster's length is the distance to the next set bit, its number the count of valid clusters below it
//                (ascending beam order, as the serial state machine numbers them); then the wrap merge as in k_circles.
//   the fit      one WAVE per cluster (waves loop when there are more clusters than waves), point k of the cluster in lane
//                k % 64.  Every sum over the points -- the means, z_sum, the three sums of a Jacobi pair, the column norms,
//                the inscribed-angle sum -- is a per-lane partial over k = lane, lane + 64, ... followed by the xor butterfly
//                32, 16, .., 1: its order depends on the point count alone, not on the wave, the cluster's number or its place
//                in the scan, and every lane ends with the same bits, so all 4 x 4 work (V, Y, Q, the symmetric eigen-solve,
//                the back-substitution) is wave-uniform and branch decisions are scalar.  Each lane rotates its own rows.
//   LDS          r, x, y [nb] and the design matrices, 4 nb doubles, COLUMN-major per cluster (column j of cluster c at
//                4 zoff[c] + j m): lanes reading one column of consecutive points read consecutive doubles, no bank is
//                hit twice.  7 nb doubles dynamic (56 KiB at 1024 beams) + 6.3 KiB static.
// Four waves, one per SIMD of the compute unit: the critical path of a tube-world scan is its largest wall cluster (50 to 90
// points), a latency-bound chain (LDS round trip, cross-lane butterfly, sqrt / division) that a second wave on the same SIMD
// would only share issue slots with, and the wave-uniform 4 x 4 state of the fit (V, Q, E, the rotations fully unrolled so
// that every index is static) asks for 287 registers: one wave per SIMD has 512 (256 VGPRs + AGPRs), two would spill.
// No atomics, no scratch, no inline assembly; -ffp-contract=off like the rest of the library.
#include "ekf_kernels.hpp"
#include "ekf_dense.hpp"

namespace ekf {

namespace {

constexpr int kScanWaves = 4, kScanThreads = kScanWaves * kWave;
constexpr int kScanMaxBeams = kDense64ScanMaxBeams, kScanMaxClusters = kDense64ScanMaxClusters;
constexpr int kScanWords = kScanMaxBeams / kWave;                 // ballot words of a scan
constexpr int kScanPasses = kScanWords / kScanWaves;              // words per wave
static_assert(kScanWords % kScanWaves == 0 && kScanMaxClusters == 2 * kWave, "the ballot passes and the output pass");

struct ScanCluster {
    int n, s0, l0, s1, l1;  // points; segment 0 (start, len), segment 1 (start, len) after a wrap merge
};

__device__ __forceinline__ int sc_beam(const ScanCluster& c, int k) { return k < c.l0 ? c.s0 + k : c.s1 + (k - c.l0); }

// the fixed butterfly: every lane ends with the same bits (a + b == b + a)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ void wave_sum3(double& a, double& b, double& c) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ta = __shfl_xor(a, d), tb = __shfl_xor(b, d), tc = __shfl_xor(c, d);
        a += ta; b += tb; c += tc;
    }
}
// a decision every lane takes alike (its operands are wave-uniform bit for bit), as a scalar
__device__ __forceinline__ bool uniform(bool b) { return __builtin_amdgcn_readfirstlane(b ? 1 : 0) != 0; }

// one-sided Jacobi SVD of the m x 4 matrix Z (column-major, column j at Z + j m), the rows k = lane, lane + 64, .. this
// lane's; s, V wave-uniform.  cf_svd4 of ekf_circles.hip with the sums over the wave.
__device__ __forceinline__ void sc_svd4(double* Z, int m, int lane, double (&s)[4], double (&V)[16]) {
#pragma unroll
    for (int i = 0; i < 16; i++) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double* Zp = Z + p * m;
                double* Zq = Z + q * m;
                double alpha = 0.0, beta = 0.0, gamma = 0.0;
                for (int k = lane; k < m; k += kWave) {
                    const double zp = Zp[k], zq = Zq[k];
                    alpha += zp * zp; beta += zq * zq; gamma += zp * zq;
                }
                wave_sum3(alpha, beta, gamma);
                const double lim = sqrt(alpha * beta);
                if (uniform(gamma == 0.0 || fabs(gamma) <= 1e-300 || fabs(gamma) <= 1e-17 * lim)) continue;
                if (fabs(gamma) > off) off = fabs(gamma) / (lim > 0 ? lim : 1.0);
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int k = lane; k < m; k += kWave) {
                    const double zp = Zp[k], zq = Zq[k];
                    Zp[k] = c * zp - sn * zq;
                    Zq[k] = sn * zp + c * zq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double vp = V[4 * k + p], vq = V[4 * k + q];
                    V[4 * k + p] = c * vp - sn * vq;
                    V[4 * k + q] = sn * vp + c * vq;
                }
            }
        if (uniform(off < 1e-15)) break;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double a = 0.0;
        for (int k = lane; k < m; k += kWave) a += Z[j * m + k] * Z[j * m + k];
        s[j] = sqrt(wave_sum(a));
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

// cf_eig4_sym of ekf_circles.hip, every index static: A, w, E stay in registers
__device__ __forceinline__ void sc_eig4_sym(double (&A)[16], double (&w)[4], double (&E)[16]) {
#pragma unroll
    for (int i = 0; i < 16; i++) E[i] = (i % 5 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0.0, diag = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            diag += A[5 * i] * A[5 * i];
#pragma unroll
            for (int j = i + 1; j < 4; j++) off += A[4 * i + j] * A[4 * i + j];
        }
        if (uniform(off <= 1e-34 * diag || off == 0.0)) break;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[4 * p + q];
                if (uniform(apq == 0.0)) continue;
                const double theta = (A[5 * q] - A[5 * p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(1.0 + theta * theta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double akp = A[4 * k + p], akq = A[4 * k + q];
                    A[4 * k + p] = c * akp - sn * akq;
                    A[4 * k + q] = sn * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double apk = A[4 * p + k], aqk = A[4 * q + k];
                    A[4 * p + k] = c * apk - sn * aqk;
                    A[4 * q + k] = sn * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double ekp = E[4 * k + p], ekq = E[4 * k + q];
                    E[4 * k + p] = c * ekp - sn * ekq;
                    E[4 * k + q] = sn * ekp + c * ekq;
                }
            }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = A[5 * i];
}

// head [2] = {circles kept, clusters}; centres [max_out][2], radii [max_out] the first max_out circles in cluster order;
// all_out [clusters][4] = x, y, r, is_circle of every cluster
__global__ __launch_bounds__(kScanThreads) void k_scan_circles(const double* __restrict__ ranges, int nb, int max_out,
                                                               int* __restrict__ head, double* __restrict__ centres,
                                                               double* __restrict__ radii, double* __restrict__ all_out) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* r = sm;            // [nb]
    double* xs = r + nb;       // [nb]
    double* ys = xs + nb;      // [nb]
    double* Zb = ys + nb;      // [4 nb] design matrices, partitioned by cluster, column-major inside a cluster
    __shared__ ScanCluster cl[kScanMaxClusters];
    __shared__ int zoff[kScanMaxClusters];
    __shared__ double res[kScanMaxClusters][4];
    __shared__ unsigned long long start_w[kScanWords], valid_w[kScanWords], keep_w[2];
    __shared__ int nc_sh;

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const double angle_resolution = 2 * kPI / (double)nb;  // circle_fitting.cpp:16
    for (int i = tid; i < nb; i += kScanThreads) {
        const double ri = ranges[i];
        r[i] = ri;
        if (i == 0) { xs[0] = ri * cos(0.0); ys[0] = ri * sin(0.0); }           // :25-26
        else {
            const double a = normalize_angle(i * angle_resolution);            // :44-45
            xs[i] = ri * cos(a);
            ys[i] = ri * sin(a);
        }
    }
    __syncthreads();

    // clusteringRanges(), :11-90.  Beam i starts a run when i == 0, when |r[i] - r[i-1]| < 0.2 fails (a NaN fails it), or
    // when i == nb - 1 (the `i != nb-1` boundary); the run from nb - 1 is never pushed, a run of more than 6 beams is.
#pragma unroll
    for (int ps = 0; ps < kScanPasses; ps++) {
        const int w = wave + ps * kScanWaves, i = w * kWave + lane;
        const bool st = i < nb && (i == 0 || !(fabs(r[i] - r[i > 0 ? i - 1 : 0]) < 0.2) || i == nb - 1);
        const unsigned long long word = __ballot(st);
        if (lane == 0) start_w[w] = word;
    }
    __syncthreads();
    int len_of[kScanPasses];
#pragma unroll
    for (int ps = 0; ps < kScanPasses; ps++) {
        const int w = wave + ps * kScanWaves, i = w * kWave + lane;
        int len = 0;
        if (i < nb - 1 && ((start_w[w] >> lane) & 1ull)) {   // (a start below nb - 1 has the start at nb - 1 above it)
            unsigned long long above = lane < kWave - 1 ? start_w[w] >> (lane + 1) : 0ull;
            int next = i + 1, ww = w;
            while (above == 0ull && ww + 1 < kScanWords) { ww++; next = ww * kWave; above = start_w[ww]; }
            next += __ffsll((long long)above) - 1;
            len = next - i;
        }
        len_of[ps] = len;
        const unsigned long long word = __ballot(len > 6);   // the "> 6 points" rule
        if (lane == 0) valid_w[w] = word;
    }
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int ps = 0; ps < kScanPasses; ps++) {
        const int w = wave + ps * kScanWaves, i = w * kWave + lane;
        if (len_of[ps] > 6) {
            int idx = __popcll(valid_w[w] & ((1ull << lane) - 1ull));
            for (int ww = 0; ww < w; ww++) idx += __popcll(valid_w[ww]);
            if (idx < kScanMaxClusters) cl[idx] = ScanCluster{len_of[ps], i, len_of[ps], 0, 0};
        }
    }
    if (tid == 0) {
        for (int ww = 0; ww < kScanWords; ww++) total += __popcll(valid_w[ww]);
        nc_sh = total < kScanMaxClusters ? total : kScanMaxClusters;
    }
    __syncthreads();
    if (tid == 0) {
        int nc = nc_sh;
        if (nc > 0) {  // :54-70 (an empty list is UB in the reference; here: no circles)
            const double first_elem_of_first = r[cl[0].s0];
            const ScanCluster last = cl[nc - 1];
            const double last_elem_of_last = r[last.s0 + last.l0 - 1];
            if (fabs(first_elem_of_first - last_elem_of_last) < 0.2) {
                if (nc == 1) nc = 0;  // prepended to itself, then popped
                else {
                    cl[0] = ScanCluster{last.l0 + cl[0].l0, last.s0, last.l0, cl[0].s0, cl[0].l0};
                    nc--;
                }
            }
        }
        int off = 0;
        for (int c = 0; c < nc; c++) { zoff[c] = off; off += cl[c].n; }   // (the merged clusters are disjoint: off <= nb)
        nc_sh = nc;
    }
    __syncthreads();
    const int nc = nc_sh;

    for (int c = wave; c < nc; c += kScanWaves) {  // circleRegression() + classifyCircle(), one wave per cluster
        const ScanCluster cc = cl[c];
        const int m = cc.n;
        double* Z = Zb + 4 * (size_t)zoff[c];
        double x_sum = 0.0, y_sum = 0.0, dummy = 0.0;
        for (int k = lane; k < m; k += kWave) { const int bi = sc_beam(cc, k); x_sum += xs[bi]; y_sum += ys[bi]; }  // :112-117
        wave_sum3(x_sum, y_sum, dummy);
        const double x_mean = x_sum / (double)m, y_mean = y_sum / (double)m;
        double z_sum = 0.0;
        for (int k = lane; k < m; k += kWave) {                                                    // :124-141
            const int bi = sc_beam(cc, k);
            const double x = xs[bi] - x_mean, y = ys[bi] - y_mean;
            const double zi = x * x + y * y;
            z_sum += zi;
            Z[k] = zi; Z[m + k] = x; Z[2 * m + k] = y; Z[3 * m + k] = 1.0;
        }
        z_sum = wave_sum(z_sum);
        const double z_mean = z_sum / (double)m;
        double sv[4], V[16], A[4];
        sc_svd4(Z, m, lane, sv, V);                                                                // :168
        if (uniform(sv[3] < 1e-12)) {                                                              // :171-175
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
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    double a = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; k++) a += Y[4 * i + k] * Hinv[4 * k + j];
                    T[4 * i + j] = a;
                }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    double a = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; k++) a += T[4 * i + k] * Y[4 * k + j];
                    Q[4 * i + j] = a;
                }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = i + 1; j < 4; j++) { const double a = 0.5 * (Q[4 * i + j] + Q[4 * j + i]); Q[4 * i + j] = a; Q[4 * j + i] = a; }
            sc_eig4_sym(Q, w, E);                                                                  // :184
            double best = 1000.0;                                                                  // :187-197
            double As[4] = {E[0], E[4], E[8], E[12]}, tmp[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const bool take = w[e] > 0 && w[e] < best;
                best = take ? w[e] : best;
#pragma unroll
                for (int k = 0; k < 4; k++) As[k] = take ? E[4 * k + e] : As[k];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {                                                          // :211
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
        const double a = -A[1] / (2 * A[0]);                                                       // :220-222
        const double bq = -A[2] / (2 * A[0]);
        const double R_sqr = (A[1] * A[1] + A[2] * A[2] - 4 * A[0] * A[3]) / (4 * (A[0] * A[0]));
        const double cx = a + x_mean, cy = bq + y_mean, rad = sqrt(R_sqr);
        // classifyCircle(), :234-296
        const int b1 = sc_beam(cc, 0), b2 = sc_beam(cc, m - 1);
        const double p1x = xs[b1], p1y = ys[b1], p2x = xs[b2], p2y = ys[b2];
        double sum_angle = 0.0;
        for (int k = lane; k < m - 1; k += kWave) {
            if (k < 1) continue;
            const int bi = sc_beam(cc, k);
            const double pp1x = p1x - xs[bi], pp1y = p1y - ys[bi], pp2x = p2x - xs[bi], pp2y = p2y - ys[bi];
            const double top_part = pp1x * pp2x + pp1y * pp2y;
            const double bot_part = sqrt(pp1x * pp1x + pp1y * pp1y) * sqrt(pp2x * pp2x + pp2y * pp2y);
            sum_angle += acos(top_part / bot_part);
        }
        sum_angle = wave_sum(sum_angle);
        const double mean_angle = sum_angle / (m - 2);
        const int ok = (mean_angle > 1.5708 && mean_angle < 2.3562 && rad < 0.2) ? 1 : 0;           // :264-271
        if (lane == 0) { res[c][0] = cx; res[c][1] = cy; res[c][2] = rad; res[c][3] = (double)ok; }
    }
    __syncthreads();
    // :284-291 keep the classified circles, in cluster order: cluster c in thread c of the first two waves
    if (tid < kScanMaxClusters) {
        const bool kept = tid < nc && res[tid][3] != 0.0;
        const unsigned long long word = __ballot(kept);
        if (lane == 0) keep_w[wave] = word;
    }
    __syncthreads();
    if (tid < kScanMaxClusters) {
        if (tid < nc) {
#pragma unroll
            for (int k = 0; k < 4; k++) all_out[(size_t)tid * 4 + k] = res[tid][k];
            if (res[tid][3] != 0.0) {
                const int pos = __popcll(keep_w[wave] & ((1ull << lane) - 1ull)) + (wave == 1 ? __popcll(keep_w[0]) : 0);
                if (pos < max_out) {
                    centres[2 * pos] = res[tid][0];
                    centres[2 * pos + 1] = res[tid][1];
                    radii[pos] = res[tid][2];
                }
            }
        }
        if (tid == 0) {
            const int kept = __popcll(keep_w[0]) + __popcll(keep_w[1]);
            head[0] = kept < max_out ? kept : max_out;
            head[1] = nc;
        }
    }
}

}  // namespace

// ranges [nb] on the device, 1 <= nb <= 1024, 1 <= max_out <= 128 (the launcher does not check); one workgroup
void launch_dense64_scan_circles(const double* ranges, int nb, int max_out, int* head, double* centres, double* radii,
                                 double* all_out, hipStream_t st) {
    const size_t lds = sizeof(double) * (size_t)nb * 7;
    hipLaunchKernelGGL(k_scan_circles, dim3(1), dim3(kScanThreads), lds, st, ranges, nb, max_out, head, centres, radii,
                       all_out);
}

}  // namespace ekf
