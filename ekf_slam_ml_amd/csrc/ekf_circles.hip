// ekf_circles.hip -- batched rigid2d::CircleFitting on gfx950: the
// perception front end that turns 360-beam laser scans into the (x, y) measurements consumed by
// EKF_SLAM::data_association (rigid2d/src/circle_fitting.cpp:11-304, called from
// nuslam/src/landmarks.cpp:141).  One wavefront per scan: beams are spread over the 64 lanes for the
// polar -> Cartesian conversion, lane 0 runs the (inherently sequential, 360-step) clustering state
// machine with all of the reference's quirks, then one LANE per cluster does the algebraic circle fit
// and the inscribed-angle classification: cf_fit of ekf_circle_fit.hpp under LanePolicy (serial sums, the
// m x 4 design matrix row-major in the lane's own piece of LDS).  This file owns the state machine, the
// cluster-to-lane loop, the output pass and the launcher.  Tiny matrices, no reuse: latency-bound by
// construction; throughput comes from many scans in flight (grid = scans).
#include "ekf_circle_fit.hpp"

namespace ekf {

__global__ __launch_bounds__(64) void k_circles(const double* __restrict__ ranges, int nb, int max_out,
                                                double* __restrict__ centres, double* __restrict__ radii,
                                                int* __restrict__ counts, double* __restrict__ all_out,
                                                int* __restrict__ n_clusters) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double* r = sm;            // [nb]
    double* xs = r + nb;       // [nb]
    double* ys = xs + nb;      // [nb]
    double* Zb = ys + nb;      // [nb][4] design-matrix rows, partitioned by cluster
    __shared__ Cluster cl[kMaxClusters];
    __shared__ int zoff[kMaxClusters];
    __shared__ double res[kMaxClusters][4];
    __shared__ int nc_sh;

    const int s = blockIdx.x, lane = threadIdx.x;
    const double* rg = ranges + (size_t)s * nb;
    for (int i = lane; i < nb; i += 64) cf_polar(rg[i], i, nb, r, xs, ys);
    __syncthreads();

    if (lane == 0) {  // clusteringRanges(), :11-90
        int nc = 0, cur_start = 0, cur_len = 1;
        for (int i = 1; i < nb; i++) {
            if ((fabs(r[i] - r[i - 1]) < kClusterThres) && (i != (nb - 1))) {
            } else {
                if (cur_len > 6 && nc < kMaxClusters) { cl[nc] = Cluster{cur_len, cur_start, cur_len, 0, 0}; nc++; }
                cur_start = i; cur_len = 0;
            }
            cur_len++;
        }
        nc_sh = cf_wrap_merge(cl, nc, r, zoff);
    }
    __syncthreads();
    const int nc = nc_sh;

    for (int c = lane; c < nc; c += 64) {  // circleRegression() + classifyCircle(), one lane per cluster
        const Cluster cc = cl[c];
        double out[4];
        cf_fit(LanePolicy{}, cc, xs, ys, Zb + 4 * (size_t)zoff[c], out);
        for (int k = 0; k < 4; k++) res[c][k] = out[k];
    }
    __syncthreads();
    if (lane == 0) {  // :284-291 keep the classified circles, in cluster order
        int count = 0;
        for (int c = 0; c < nc; c++) {
            if (all_out) for (int k = 0; k < 4; k++) all_out[((size_t)s * kMaxClusters + c) * 4 + k] = res[c][k];
            if (res[c][3] != 0.0 && count < max_out) {
                centres[((size_t)s * max_out + count) * 2] = res[c][0];
                centres[((size_t)s * max_out + count) * 2 + 1] = res[c][1];
                radii[(size_t)s * max_out + count] = res[c][2];
                count++;
            }
        }
        counts[s] = count;
        if (n_clusters) n_clusters[s] = nc;
    }
}

int circles_max_beams() { return kMaxBeams; }
int circles_max_clusters() { return kMaxClusters; }

void launch_circles(const double* ranges, int S, int nb, int max_out, double* centres, double* radii, int* counts,
                    double* all_out, int* n_clusters, hipStream_t s) {
    const size_t lds = sizeof(double) * (size_t)nb * 7;
    hipLaunchKernelGGL(k_circles, dim3(S), dim3(64), lds, s, ranges, nb, max_out, centres, radii, counts, all_out,
                       n_clusters);
}

}  // namespace ekf
