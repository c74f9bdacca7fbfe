// ekf_dense64_health.hip -- is the covariance of the dense fp64 handle still a covariance, and the exact repair of its
// symmetry (gfx950, wave64).  Every call of the handle keeps the contract "Sigma is never symmetrised", so rounding lets
// Sigma[i][j] and Sigma[j][i] drift apart; ekf_dense64_health measures that (and the signs of the diagonal, the 2 x 2
// principal minors, what is not finite) in ONE read of the live corner, ekf_dense64_symmetrize sets both entries of every
// pair that differs in bits to fl(0.5 fl(Sigma[i][j] + Sigma[j][i])) in place.  The definitions are include/ekfslam.h's.
//   k_dh_tile<fix> a short-lived workgroup per tile pair (A <= B) of the corner, kDense64HealthTile = 64 states a side, 4096
//                 pairs, sixteen to a lane (lane = j within the tile, so a wave's loads and stores run along a row of
//                 Sigma).  Sigma[A rows, B cols] comes straight from memory.  Sigma[B rows, A cols] would be a walk down a
//                 column, so that tile is loaded as 64 row segments of 512 bytes (every load of both tiles issued before
//                 the first is used), put into LDS and read back transposed with a row stride of 65 doubles: the 32 lanes
//                 of half a wave then fall on 64 different banks.  Loads are masked element by element: nothing at an
//                 index >= Na is read.  The diagonal tile (A = B) takes its own upper triangle.
//                   fix = false: the counts (non-finite entries, pairs that differ in bits, negative 2 x 2 minors) go wave
//                 -> workgroup -> one INTEGER atomic each; the largest |d| -- on its bit pattern, so a NaN sorts above
//                 infinity -- and the lowest (i, j) that attains it are one record per tile pair.  The diagonal entries
//                 come from the [Na] copy that k_dh_diag made: two contiguous loads instead of 128 scattered ones.
//                   fix = true: the pairs that differ are counted, the maximum is one integer atomic (no location), the
//                 upper entry is stored from the register along its row, the lower one goes back into LDS at its
//                 transposed place, and after a barrier the tile is walked along rows again: an element whose bits changed
//                 is stored.  No store walks down a column; a pair that held the same bits is not written; the diagonal
//                 never.  One workgroup owns both tiles of its pair, so nothing is staged outside LDS.
//   k_dh_diag     a thread per diagonal entry: the copy for the minors, the count of entries that are NaN or <= 0, and per
//                 workgroup one record (smallest value that is not a NaN, lowest index on equal values).
//   k_dh_fold     one workgroup folds the records of the tile pairs and of the diagonal.  Both folds are pure functions of
//                 the data ("larger bits, then lower (i, j)" / "smaller value, then lower index, a NaN never"), so the
//                 result does not depend on the order of arrival.
// No floating-point atomics, no waits inside a kernel: a run repeats bit for bit.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

namespace {

typedef unsigned long long u64;

constexpr int kT = kDense64HealthTile;       // states of a tile side
constexpr int kThreads = kDense64HealthThreads;
constexpr int kRows = kThreads / kT;         // rows of a tile in flight per step: one per wave
constexpr int kPer = kT / kRows;             // elements of a tile per thread
constexpr int kLd = kT + 1;                  // LDS row stride: odd, the transposed 8-byte reads of half a wave are conflict-free
constexpr int kFoldThreads = 1024;             // one workgroup: a dozen records per thread at N = 10003
constexpr u64 kNoLoc = ~0ull;
static_assert(kT == 64 && kThreads == 256 && kPer == 16, "a wave per row of the tile, lane = column");

__device__ __forceinline__ u64 bits_of(double x) { return (u64)__double_as_longlong(x); }
__device__ __forceinline__ u64 abs_bits(double x) { return bits_of(x) & 0x7fffffffffffffffull; }
__device__ __forceinline__ bool nonfinite(double x) { return abs_bits(x) >= 0x7ff0000000000000ull; }
// does (m, loc) beat (bm, bl)?  loc = i << 32 | j, kNoLoc: no pair
__device__ __forceinline__ bool asym_better(u64 m, u64 loc, u64 bm, u64 bl) {
    return loc != kNoLoc && (bl == kNoLoc || m > bm || (m == bm && loc < bl));
}
// does the diagonal entry (d, i) beat (bd, bi)?  bi < 0: nothing yet.  A NaN never does.
__device__ __forceinline__ bool diag_better(double d, int i, double bd, int bi) {
    return d == d && i >= 0 && (bi < 0 || d < bd || (d == bd && i < bi));
}

// the tile pair of a workgroup: k = B (B + 1) / 2 + A, A <= B
__device__ __forceinline__ void tile_pair(int k, int* A, int* B) {
    int b = (int)((sqrt(8.0 * k + 1.0) - 1.0) * 0.5);
    while ((b + 1) * (b + 2) / 2 <= k) b++;
    while (b * (b + 1) / 2 > k) b--;
    *B = b;
    *A = k - b * (b + 1) / 2;
}

// words: kDense64HealthWords 64-bit words, zero before the launch (see ekf_dense.hpp).  rec_max, rec_loc: one per tile pair
// (fix = false only).  diag: [Na] (fix = false only).
template <bool kFix>
__global__ __launch_bounds__(kThreads) void k_dh_tile(double* __restrict__ S, int ld, int Na, const double* __restrict__ diag,
                                                      u64* __restrict__ words, u64* __restrict__ rec_max,
                                                      u64* __restrict__ rec_loc) {
    __shared__ double Ls[kT * kLd];
    __shared__ u64 wcnt[kThreads / 64][3], wmax[kThreads / 64], wloc[kThreads / 64];
    const int t = threadIdx.x, c = t & (kT - 1), w = t / kT;
    int A, B;
    tile_pair(blockIdx.x, &A, &B);
    const int gj = kT * B + c;   // this lane's column of the upper tile, its j
    const int lc = kT * A + c;   // this lane's column of the lower tile

    double up[kPer], lo[kPer];
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int r = w + kRows * u;
        const int gi = kT * A + r, lr = kT * B + r;
        up[u] = (gi < Na && gj < Na) ? S[(size_t)gi * ld + gj] : 0.0;
        lo[u] = (lr < Na && lc < Na) ? S[(size_t)lr * ld + lc] : 0.0;
    }
    double dj = 0.0;
    if (!kFix && gj < Na) dj = diag[gj];
#pragma unroll
    for (int u = 0; u < kPer; u++) Ls[(w + kRows * u) * kLd + c] = lo[u];
    __syncthreads();

    u64 n_nonfinite = 0, n_asym = 0, n_minor = 0, most = 0, loc = kNoLoc;
    if (!kFix) {   // every entry of the two tiles once (the diagonal tile is one tile); what the mask left out is 0.0
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            if (nonfinite(lo[u])) n_nonfinite++;
            if (A != B && nonfinite(up[u])) n_nonfinite++;
        }
    }
#pragma unroll
    for (int u = 0; u < kPer; u++) {
        const int r = w + kRows * u;
        const int gi = kT * A + r;
        if (!(gi < gj && gj < Na)) continue;
        const double a = up[u], b = Ls[c * kLd + r];   // Sigma[i][j], Sigma[j][i]
        const bool differ = bits_of(a) != bits_of(b);
        if (differ) n_asym++;
        const u64 m = abs_bits(a - b);
        if (kFix) {
            most = m > most ? m : most;
            if (differ) {
                const double v = 0.5 * (a + b);
                S[(size_t)gi * ld + gj] = v;
                Ls[c * kLd + r] = v;
            }
        } else {
            const u64 here = ((u64)(unsigned)gi << 32) | (u64)(unsigned)gj;
            if (asym_better(m, here, most, loc)) most = m, loc = here;
            const double di = diag[gi];   // (the same address across the wave)
            if (a * b > di * dj) n_minor++;
        }
    }
    if (kFix) {   // the lower tile goes back the way it came: along rows, only what changed
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kPer; u++) {
            const int r = w + kRows * u;
            const int lr = kT * B + r;
            const double v = Ls[r * kLd + c];
            if (lr < Na && lc < Na && bits_of(v) != bits_of(lo[u])) S[(size_t)lr * ld + lc] = v;
        }
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_nonfinite += __shfl_down(n_nonfinite, off);
        n_asym += __shfl_down(n_asym, off);
        n_minor += __shfl_down(n_minor, off);
        const u64 om = __shfl_down(most, off), ol = __shfl_down(loc, off);
        if (kFix) most = om > most ? om : most;
        else if (asym_better(om, ol, most, loc)) most = om, loc = ol;
    }
    if (c == 0) {
        wcnt[w][0] = n_nonfinite, wcnt[w][1] = n_asym, wcnt[w][2] = n_minor;
        wmax[w] = most, wloc[w] = loc;
    }
    __syncthreads();
    if (t == 0) {
        for (int h = 1; h < kThreads / 64; h++) {
            n_nonfinite += wcnt[h][0], n_asym += wcnt[h][1], n_minor += wcnt[h][2];
            if (kFix) most = wmax[h] > most ? wmax[h] : most;
            else if (asym_better(wmax[h], wloc[h], most, loc)) most = wmax[h], loc = wloc[h];
        }
        if (n_nonfinite) atomicAdd(words + kDense64HealthNonfinite, n_nonfinite);
        if (n_asym) atomicAdd(words + kDense64HealthAsym, n_asym);
        if (n_minor) atomicAdd(words + kDense64HealthMinor, n_minor);
        if (kFix) {
            if (most) atomicMax(words + kDense64HealthMaxBits, most);
        } else {
            rec_max[blockIdx.x] = most;
            rec_loc[blockIdx.x] = loc;
        }
    }
}

// diag [Na] <- the diagonal; words[kDense64HealthDiagBad] += entries that are NaN or <= 0; one record per workgroup
__global__ __launch_bounds__(kThreads) void k_dh_diag(const double* __restrict__ S, int ld, int Na, double* __restrict__ diag,
                                                      u64* __restrict__ words, double* __restrict__ drec_val,
                                                      int* __restrict__ drec_idx) {
    __shared__ double sv[kThreads / 64];
    __shared__ int si[kThreads / 64];
    __shared__ unsigned int sb[kThreads / 64];
    const int t = threadIdx.x, i = kThreads * blockIdx.x + t;
    double bd = __builtin_huge_val();
    int bi = -1;
    unsigned int bad = 0;
    if (i < Na) {
        const double d = S[(size_t)i * ld + i];
        diag[i] = d;
        if (!(d > 0.0)) bad = 1;
        if (d == d) bd = d, bi = i;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        bad += __shfl_down(bad, off);
        const double od = __shfl_down(bd, off);
        const int oi = __shfl_down(bi, off);
        if (diag_better(od, oi, bd, bi)) bd = od, bi = oi;
    }
    if ((t & 63) == 0) sv[t >> 6] = bd, si[t >> 6] = bi, sb[t >> 6] = bad;
    __syncthreads();
    if (t == 0) {
        for (int h = 1; h < kThreads / 64; h++) {
            bad += sb[h];
            if (diag_better(sv[h], si[h], bd, bi)) bd = sv[h], bi = si[h];
        }
        if (bad) atomicAdd(words + kDense64HealthDiagBad, (u64)bad);
        drec_val[blockIdx.x] = bd;
        drec_idx[blockIdx.x] = bi;
    }
}

// words[MaxBits], [MaxLoc], [MinDiag], [MinDiagIdx] <- the folds of the records
__global__ __launch_bounds__(kFoldThreads) void k_dh_fold(const u64* __restrict__ rec_max, const u64* __restrict__ rec_loc, int n_rec,
                                                      const double* __restrict__ drec_val, const int* __restrict__ drec_idx,
                                                      int n_drec, u64* __restrict__ words) {
    __shared__ u64 sm[kFoldThreads], sl[kFoldThreads];
    __shared__ double sv[kFoldThreads];
    __shared__ int si[kFoldThreads];
    const int t = threadIdx.x;
    u64 most = 0, loc = kNoLoc;
    for (int k = t; k < n_rec; k += kFoldThreads)
        if (asym_better(rec_max[k], rec_loc[k], most, loc)) most = rec_max[k], loc = rec_loc[k];
    double bd = __builtin_huge_val();
    int bi = -1;
    for (int k = t; k < n_drec; k += kFoldThreads)
        if (diag_better(drec_val[k], drec_idx[k], bd, bi)) bd = drec_val[k], bi = drec_idx[k];
    sm[t] = most, sl[t] = loc, sv[t] = bd, si[t] = bi;
    __syncthreads();
    for (int half = kFoldThreads / 2; half > 0; half >>= 1) {
        if (t < half) {
            if (asym_better(sm[t + half], sl[t + half], sm[t], sl[t])) sm[t] = sm[t + half], sl[t] = sl[t + half];
            if (diag_better(sv[t + half], si[t + half], sv[t], si[t])) sv[t] = sv[t + half], si[t] = si[t + half];
        }
        __syncthreads();
    }
    if (t == 0) {
        words[kDense64HealthMaxBits] = sl[0] == kNoLoc ? 0 : sm[0];
        words[kDense64HealthMaxLoc] = sl[0];
        words[kDense64HealthMinDiag] = bits_of(si[0] < 0 ? __builtin_huge_val() : sv[0]);
        words[kDense64HealthMinDiagIdx] = (u64)(long long)si[0];
    }
}

}  // namespace

Dense64HealthPlan dense64_health_plan(int Na) {
    Dense64HealthPlan p{};
    p.Na = Na;
    p.tiles = (Na + kT - 1) / kT;
    p.pairs = (size_t)p.tiles * (p.tiles + 1) / 2;
    p.diag_groups = (Na + kThreads - 1) / kThreads;
    p.off_words = 0;
    p.off_diag = sizeof(u64) * kDense64HealthWords;
    p.off_rec_max = p.off_diag + sizeof(double) * (size_t)p.tiles * kT;
    p.off_rec_loc = p.off_rec_max + sizeof(u64) * p.pairs;
    p.off_drec_val = p.off_rec_loc + sizeof(u64) * p.pairs;
    p.off_drec_idx = p.off_drec_val + sizeof(double) * p.diag_groups;
    p.bytes = p.off_drec_idx + sizeof(int) * p.diag_groups;
    return p;
}

void launch_dense64_health(const Dense64HealthPlan& p, const double* Sigma, int ld, void* ws, hipStream_t st) {
    char* b = static_cast<char*>(ws);
    u64* words = reinterpret_cast<u64*>(b + p.off_words);
    double* diag = reinterpret_cast<double*>(b + p.off_diag);
    u64* rec_max = reinterpret_cast<u64*>(b + p.off_rec_max);
    u64* rec_loc = reinterpret_cast<u64*>(b + p.off_rec_loc);
    double* drec_val = reinterpret_cast<double*>(b + p.off_drec_val);
    int* drec_idx = reinterpret_cast<int*>(b + p.off_drec_idx);
    hipLaunchKernelGGL(k_dh_diag, dim3(p.diag_groups), dim3(kThreads), 0, st, Sigma, ld, p.Na, diag, words, drec_val, drec_idx);
    hipLaunchKernelGGL(k_dh_tile<false>, dim3((unsigned)p.pairs), dim3(kThreads), 0, st, const_cast<double*>(Sigma), ld, p.Na,
                       diag, words, rec_max, rec_loc);
    hipLaunchKernelGGL(k_dh_fold, dim3(1), dim3(kFoldThreads), 0, st, rec_max, rec_loc, (int)p.pairs, drec_val, drec_idx,
                       p.diag_groups, words);
}

void launch_dense64_symmetrize(const Dense64HealthPlan& p, double* Sigma, int ld, void* ws, hipStream_t st) {
    u64* words = reinterpret_cast<u64*>(static_cast<char*>(ws) + p.off_words);
    hipLaunchKernelGGL(k_dh_tile<true>, dim3((unsigned)p.pairs), dim3(kThreads), 0, st, Sigma, ld, p.Na,
                       static_cast<const double*>(nullptr), words, static_cast<u64*>(nullptr), static_cast<u64*>(nullptr));
}

}  // namespace ekf
