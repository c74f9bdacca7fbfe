// ekf_dense64_scan.hip -- rigid2d::CircleFitting::approxCirclePositions (circle_fitting.cpp:11-304) for ONE laser scan, shaped
// for latency: the input of the dense fp64 handle's scan calls (ekf_dense64_fit_scan, ekf_dense64_associate_scan).  It does
// what k_circles (ekf_circles.hip, one wavefront per scan, one LANE per cluster, built for thousands of scans) does, from
// the same source (ekf_circle_fit.hpp: prologue, wrap merge, the fit of one cluster), with the work of a single scan spread
// over one workgroup of four waves.  This file owns:
//   clustering   every beam computes its own boundary flag from r[i], r[i - 1]; a wave's 64 flags are one ballot word; a
//                cluster's length is the distance to the next set bit, its number the count of valid clusters below it
//                (ascending beam order, as the serial state machine numbers them); thread 0 then runs the shared wrap merge.
//   the waves    one WAVE per cluster (waves loop when there are more clusters than waves): cf_fit under WavePolicy, whose
//                sums depend on the point count alone, not on the wave, the cluster's number or its place in the scan.
//   the output   cluster c in thread c of the first two waves; a kept circle's place is the bit count below it.
//   LDS          r, x, y [nb] and the design matrices, 4 nb doubles, COLUMN-major per cluster (column j of cluster c at
//                4 zoff[c] + j m).  7 nb doubles dynamic (56 KiB at 1024 beams) + 7.3 KiB static.
// Four waves, one per SIMD of the compute unit: the critical path of a tube-world scan is its largest wall cluster (50 to 90
// points), a latency-bound chain (LDS round trip, cross-lane butterfly, sqrt / division) that a second wave on the same SIMD
// would only share issue slots with, and the wave-uniform 4 x 4 state of the fit (V, Q, E) asks for more registers than two
// waves on a SIMD could have without spilling: one wave per SIMD has 512 (256 VGPRs + AGPRs).
// No atomics, no scratch, no inline assembly; -ffp-contract=off like the rest of the library.
#include "ekf_circle_fit.hpp"
#include "ekf_dense.hpp"

namespace ekf {

namespace {

constexpr int kScanWaves = 4, kScanThreads = kScanWaves * kWave;
constexpr int kScanWords = kMaxBeams / kWave;                     // ballot words of a scan
constexpr int kScanPasses = kScanWords / kScanWaves;              // words per wave
static_assert(kScanWords % kScanWaves == 0 && kMaxClusters == 2 * kWave, "the ballot passes and the output pass");

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
    __shared__ Cluster cl[kMaxClusters];
    __shared__ int zoff[kMaxClusters];
    __shared__ double res[kMaxClusters][4];
    __shared__ unsigned long long start_w[kScanWords], valid_w[kScanWords], keep_w[2];
    __shared__ int nc_sh;

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    for (int i = tid; i < nb; i += kScanThreads) cf_polar(ranges[i], i, nb, r, xs, ys);
    __syncthreads();

    // clusteringRanges(), :11-90.  Beam i starts a run when i == 0, when |r[i] - r[i-1]| < 0.2 fails (a NaN fails it), or
    // when i == nb - 1 (the `i != nb-1` boundary); the run from nb - 1 is never pushed, a run of more than 6 beams is.
#pragma unroll
    for (int ps = 0; ps < kScanPasses; ps++) {
        const int w = wave + ps * kScanWaves, i = w * kWave + lane;
        const bool st = i < nb && (i == 0 || !(fabs(r[i] - r[i > 0 ? i - 1 : 0]) < kClusterThres) || i == nb - 1);
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
            if (idx < kMaxClusters) cl[idx] = Cluster{len_of[ps], i, len_of[ps], 0, 0};
        }
    }
    if (tid == 0) {
        for (int ww = 0; ww < kScanWords; ww++) total += __popcll(valid_w[ww]);
        nc_sh = total < kMaxClusters ? total : kMaxClusters;
    }
    __syncthreads();
    if (tid == 0) nc_sh = cf_wrap_merge(cl, nc_sh, r, zoff);
    __syncthreads();
    const int nc = nc_sh;

    for (int c = wave; c < nc; c += kScanWaves) {  // circleRegression() + classifyCircle(), one wave per cluster
        const Cluster cc = cl[c];
        double out[4];
        cf_fit(WavePolicy{lane}, cc, xs, ys, Zb + 4 * (size_t)zoff[c], out);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) res[c][k] = out[k];
        }
    }
    __syncthreads();
    // :284-291 keep the classified circles, in cluster order: cluster c in thread c of the first two waves
    if (tid < kMaxClusters) {
        const bool kept = tid < nc && res[tid][3] != 0.0;
        const unsigned long long word = __ballot(kept);
        if (lane == 0) keep_w[wave] = word;
    }
    __syncthreads();
    if (tid < kMaxClusters) {
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
