// ekf_dense64_evidence.hip -- one laser scan cast against the dense fp64 handle's OWN map (gfx950, wave64): for every beam the
// range the map predicts and the landmark it should stop on, and per landmark how many beams agree with that, went through it
// or stopped short of it.  The geometry is model 0 of the simulator (k_sim_scans of ekf_sim.hip, synth.make_scans) on the
// state's pose and landmarks, operation by operation: beam b leaves (x, y) = state[1..2] in direction state[0] + 2 pi b / n,
// r = fmin(fmin(wall_x, wall_y), range_max), then for the landmarks in ascending index  f = pose - landmark,
// bq = f . d, cq = f . f - radius^2, disc = bq bq - cq, and where disc > 0 the root t = -bq - sqrt(disc) replaces r when
// 0 < t < r -- a strict <, so of equal roots the lowest index stands, and a NaN root never wins.
//   k_dev_tol         a thread per landmark: tol = tol_abs + kappa sqrt(max(S00, 0)) from the S the sparse scoring kernel
//                     left (+Inf for a flagged S); without Sigma (kappa == 0) tol_abs.
//   k_dev_candidates  ONE workgroup of four waves: the landmarks with f . f <= (range_max + radius)^2 (1 + 1e-12)
//                     compacted into a list (index, f) in ascending index -- a ballot per wave, bit counts below the lane and over the earlier
//                     waves, as k_scan_circles numbers its clusters.  A landmark out of reach has no root below range_max,
//                     so the list changes no result; a NaN landmark fails the comparison.
//   k_dev_beams       a workgroup (one wave) per kDense64EvidenceBeamTile beams, a lane per beam: the candidates pass through
//                     LDS kDense64EvidenceLmChunk at a time, (smallest root, its index) stay in registers, then the beam is
//                     classed against the observed range and counted: per landmark by integer atomics, per call by a
//                     ballot's bit count and one integer atomic a wave.
// No floating-point atomics and no sum of floating-point values at all: every output is a pure function of its beam or an
// integer count, so a run repeats bit for bit whatever the order of the workgroups, the capacity N or the landmarks out of
// reach.  The library is built with -ffp-contract=off: products and sums are rounded separately, as numpy rounds them.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

namespace {

constexpr int kTile = kDense64EvidenceBeamTile, kChunk = kDense64EvidenceLmChunk, kThreads = kDense64EvidenceThreads;
constexpr int kCandThreads = 256, kCandWaves = kCandThreads / 64;
static_assert(kTile == kThreads && kThreads == 64 && kChunk % kThreads == 0, "a lane per beam, one wave per workgroup");

enum : int { kRepCandidates = 0, kRepOnTube = 1, kRepUnexplained = 2, kRepInvalid = 3 };

__global__ __launch_bounds__(256) void k_dev_tol(const double* __restrict__ S, const int* __restrict__ flag, int n,
                                                 double tol_abs, double kappa, double* __restrict__ tol) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = tol_abs;
    if (S) v = flag[i] ? __builtin_huge_val() : tol_abs + kappa * sqrt(fmax(S[4 * (size_t)i], 0.0));
    tol[i] = v;
}

__global__ __launch_bounds__(kCandThreads) void k_dev_candidates(const double* __restrict__ x, int first_lm, int count,
                                                                  double reach2, int* __restrict__ cand_idx,
                                                                  double* __restrict__ cand_xy, int* __restrict__ report) {
    __shared__ int wcnt[kCandWaves];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const double ox = x[1], oy = x[2];
    int n = 0;
    for (int base = 0; base < count; base += kCandThreads) {   // (uniform: every wave meets every ballot and barrier)
        const int i = base + t;
        double fx = 0.0, fy = 0.0;
        bool in = false;
        if (i < count) {
            fx = ox - x[3 + 2 * (size_t)(first_lm + i)];
            fy = oy - x[4 + 2 * (size_t)(first_lm + i)];
            in = fx * fx + fy * fy <= reach2;
        }
        const unsigned long long word = __ballot(in);
        if (lane == 0) wcnt[w] = __popcll(word);
        __syncthreads();
        int at = n + __popcll(word & ((1ull << lane) - 1ull)), total = 0;
        for (int ww = 0; ww < kCandWaves; ww++) {
            if (ww < w) at += wcnt[ww];
            total += wcnt[ww];
        }
        if (in) {   // at < count: the list is never longer than the landmarks looked at
            cand_idx[at] = first_lm + i;
            cand_xy[2 * (size_t)at] = fx;
            cand_xy[2 * (size_t)at + 1] = fy;
        }
        n += total;
        __syncthreads();
    }
    if (t == 0) report[kRepCandidates] = n;
}

__global__ __launch_bounds__(kThreads) void k_dev_beams(const double* __restrict__ x, const int* __restrict__ cand_idx,
                                                        const double* __restrict__ cand_xy, const double* __restrict__ tol,
                                                        const double* __restrict__ ranges, int first_lm, int count,
                                                        int n_beams, double range_max, double half, double r2,
                                                        double tol_abs, double* __restrict__ expected,
                                                        int* __restrict__ hit, unsigned char* __restrict__ cls,
                                                        int* __restrict__ counts, int* __restrict__ report) {
    __shared__ double sxy[2 * kChunk];
    __shared__ int sidx[kChunk];
    const int t = threadIdx.x, b = blockIdx.x * kTile + t;
    const bool live = b < n_beams;
    const int nc = report[kRepCandidates];   // (written by the launch before this one)
    const double th0 = x[0], ox = x[1], oy = x[2];
    const double ang = 2.0 * 3.141592653589793 * (double)b / (double)n_beams;
    const double th = th0 + ang;
    const double dx = cos(th), dy = sin(th);
    const double inf = __builtin_huge_val();
    const double tx = dx > 0 ? (half - ox) / dx : (dx < 0 ? (-half - ox) / dx : inf);
    const double ty = dy > 0 ? (half - oy) / dy : (dy < 0 ? (-half - oy) / dy : inf);
    double r = fmin(fmin(tx, ty), range_max);
    int win = -1;
    for (int c0 = 0; c0 < nc; c0 += kChunk) {   // (uniform)
        const int m = min(kChunk, nc - c0);
        for (int k = t; k < m; k += kThreads) {
            sidx[k] = cand_idx[c0 + k];
            sxy[2 * k] = cand_xy[2 * (size_t)(c0 + k)];
            sxy[2 * k + 1] = cand_xy[2 * (size_t)(c0 + k) + 1];
        }
        __syncthreads();
        for (int k = 0; k < m; k++) {
            const double fx = sxy[2 * k], fy = sxy[2 * k + 1];
            const double bq = fx * dx + fy * dy;
            const double cq = fx * fx + fy * fy - r2;
            const double disc = bq * bq - cq;
            if (disc > 0) {
                const double tt = -bq - sqrt(disc);
                if (tt > 0 && tt < r) { r = tt; win = sidx[k]; }
            }
        }
        __syncthreads();
    }
    // the class of the beam (include/ekfslam.h): 0 wall or range_max, 1 agree, 2 through, 3 short, 4 invalid
    int c = 0;
    bool unexplained = false, invalid = false;
    if (live && ranges) {
        const double obs = ranges[b];
        if (!(obs > 0.0)) {   // a NaN or <= 0
            c = 4;
            invalid = true;
        } else if (win < 0) {
            unexplained = obs < r - tol_abs;
        } else {
            const double tl = tol[win - first_lm], d = obs - r;
            c = fabs(d) <= tl ? 1 : (d > tl ? 2 : 3);   // (3: r - obs = -d > tl, the one case left)
            int* mine = counts + (win - first_lm);
            atomicAdd(mine, 1);
            atomicAdd(mine + (size_t)c * count, 1);
        }
    }
    if (live) {
        expected[b] = r;
        hit[b] = win;
        cls[b] = (unsigned char)c;
    }
    const int on = __popcll(__ballot(live && win >= 0)), un = __popcll(__ballot(unexplained)), bad = __popcll(__ballot(invalid));
    if (t == 0) {
        if (on) atomicAdd(report + kRepOnTube, on);
        if (un) atomicAdd(report + kRepUnexplained, un);
        if (bad) atomicAdd(report + kRepInvalid, bad);
    }
}

}  // namespace

Dense64EvidencePlan dense64_evidence_plan(int first_lm, int count) {
    Dense64EvidencePlan p{};
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t n = (size_t)count, nb = kDense64ScanMaxBeams;
    p.first_lm = first_lm;
    p.count = count;
    p.off_report = 0;
    p.off_counts = 16;   // [n_expected | n_agree | n_through | n_short], count ints each
    p.zero_bytes = 16 + sizeof(int) * 4 * n;
    p.off_tol = up(p.zero_bytes);
    p.off_cand_idx = p.off_tol + up(sizeof(double) * n);
    p.off_cand_xy = p.off_cand_idx + up(sizeof(int) * n);
    p.off_ranges = p.off_cand_xy + sizeof(double) * 2 * n;
    p.off_expected = p.off_ranges + sizeof(double) * nb;
    p.off_hit = p.off_expected + sizeof(double) * nb;
    p.off_class = p.off_hit + sizeof(int) * nb;
    p.bytes = p.off_class + nb;
    return p;
}

void launch_dense64_evidence_tol(const Dense64EvidencePlan& p, int at, int n, const double* S, const int* flag,
                                 double tol_abs, double kappa, void* ws, hipStream_t st) {
    double* tol = reinterpret_cast<double*>(static_cast<char*>(ws) + p.off_tol) + at;
    hipLaunchKernelGGL(k_dev_tol, dim3((n + 255) / 256), dim3(256), 0, st, S, flag, n, tol_abs, kappa, tol);
}

void launch_dense64_evidence(const Dense64EvidencePlan& p, const double* state, int n_beams, double range_max,
                             double border_width, double tube_radius, double tol_abs, int have_ranges, void* ws,
                             hipStream_t st) {
    char* b = static_cast<char*>(ws);
    int* report = reinterpret_cast<int*>(b + p.off_report);
    int* cand_idx = reinterpret_cast<int*>(b + p.off_cand_idx);
    double* cand_xy = reinterpret_cast<double*>(b + p.off_cand_xy);
    // a relative slack of 1e-12 on the squared reach: whatever the rounding of the sum below, a landmark whose rounded
    // root lies under range_max (|f| < range_max + radius by more than that) is in the list
    const double reach = range_max + tube_radius;
    hipLaunchKernelGGL(k_dev_candidates, dim3(1), dim3(kCandThreads), 0, st, state, p.first_lm, p.count,
                       reach * reach * (1.0 + 1e-12),
                       cand_idx, cand_xy, report);
    hipLaunchKernelGGL(k_dev_beams, dim3((n_beams + kTile - 1) / kTile), dim3(kThreads), 0, st, state, cand_idx, cand_xy,
                       reinterpret_cast<const double*>(b + p.off_tol),
                       have_ranges ? reinterpret_cast<const double*>(b + p.off_ranges) : nullptr, p.first_lm, p.count,
                       n_beams, range_max, border_width / 2.0, tube_radius * tube_radius,
                       tol_abs, reinterpret_cast<double*>(b + p.off_expected), reinterpret_cast<int*>(b + p.off_hit),
                       reinterpret_cast<unsigned char*>(b + p.off_class), reinterpret_cast<int*>(b + p.off_counts), report);
}

}  // namespace ekf
