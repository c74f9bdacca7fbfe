// ekf_dense64_pairs.hip -- the landmark-to-landmark Mahalanobis test of the dense fp64 handle at map scale (gfx950, wave64):
// for every pair a < b of the first n_lm landmarks the score d2(a, b) that ekf_dense64_score_sparse returns for
//   m = 2, s = 4, cols = {3 + 2a, 4 + 2a, 3 + 2b, 4 + 2b}, Hc = [[1, 0, -1, 0], [0, 1, 0, -1]], R = r_merge I,
//   nu = x[a] - x[b]
// bit for bit, and per landmark the partner with the smallest score.  All pairs are ONE read of Sigma's landmark corner.
//   k_dpr_tile    a short-lived workgroup per tile (A <= B) of the pair matrix, kDense64PairsTile = 32 landmarks a side,
//                 1024 pairs, four to a lane (lane = b within the tile, so a wave's loads run along a row of Sigma).  A pair
//                 needs the four 2 x 2 blocks Sigma_aa, Sigma_ab, Sigma_ba, Sigma_bb.  Sigma_ab comes straight from memory:
//                 the 32 lanes of half a wave read 512 contiguous bytes of a row (landmark columns start at the odd index 3,
//                 so the two doubles sit on an 8-byte boundary: one 16-byte access declared as such).  Sigma_ba would be a
//                 walk down a column, so the tile Sigma[B rows, A columns] goes through LDS, loaded as 64 row segments of
//                 512 bytes (lanes along the row, every load of the tile issued before the first is used) and read back
//                 transposed with a row stride of 66 doubles.  The diagonal blocks and the state are a few broadcast loads.
//                 Loads are masked element by element: nothing at an index >= 3 + 2 n_lm is read.  The per-pair arithmetic
//                 runs in registers (pair_score below).  The scores of the tile meet in LDS; 32 threads fold the rows and
//                 32 the columns in ascending index and write one (min, index) record per landmark and tile, slot-major.
//                 The two counts (d2 < gate, flagged) go wave -> workgroup -> one INTEGER atomic each.
//   k_dpr_fold    a workgroup per 32 landmarks folds each landmark's tiles + 1 records (eight groups of lanes over the
//                 slots, then LDS) into nearest[] and d2[].
//   k_dpr_terms   one thread: the operands of the merging correction, written where the sparse correction reads them: those
//                 of the pair's score with the innovation 0 - (x_lo - x_hi) = x_hi - x_lo, the exact negative of the
//                 score's nu, so S and nis keep their bits.
// THE ARITHMETIC OF A PAIR is that of k_dsp_score (ekf_dense64_sparse.hip) and gj_invert / gj_quadratic
// (ekf_dense64_invert.hpp) at m = 2, s = 4, operation by operation: T' = Hc G by four fused multiply-adds from +0 in
// ascending k, S = T' Hc^T likewise, R by one plain addition, the elimination with its pivot rule (largest |entry|, lowest
// row on a tie) and its verdict (non-finite S, zero or non-finite pivot, non-finite inverse), then S^-1 nu row by row and
// the dot product from 0.0, products and sums rounded separately (the library is built with -ffp-contract=off).  Only
// values nothing reads are left out (columns 0 and 1 of the augmented matrix once they are eliminated).
// The argmin is the pure function "smaller score, then lower index, a NaN never wins", so every order of folding gives the
// same bits; no floating-point atomics anywhere: a run repeats bit for bit.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

namespace {

constexpr int kTL = kDense64PairsTile;   // landmarks of a tile side
constexpr int kTS = 2 * kTL;             // states of a tile side
constexpr int kThreads = kDense64PairsThreads;
constexpr int kPer = kTL * kTL / kThreads;   // pairs of a lane
constexpr int kLdq = kTS + 2;                // LDS row stride of the Sigma_ba tile: even (16-byte reads), 2-way at worst
constexpr int kRes = kTL + 1;                // row stride of the tile's scores: conflict-free along rows and columns
constexpr int kFill = kTS * kTS / kThreads;  // elements of the staged tile per thread
constexpr int kFoldGroups = kThreads / kTL;
static_assert(kTL == 32 && kThreads == 256 && kPer == 4, "lane = (a & 7 .. , b): half a wave per row of pairs");

// two doubles that sit on an 8-byte boundary only (landmark i starts at 3 + 2 i): one 16-byte access
typedef double pair8 __attribute__((ext_vector_type(2), aligned(8)));
typedef double pair16 __attribute__((ext_vector_type(2)));

// does (d, i) beat the best so far (bd, bi)?  bi < 0: nothing yet.  A NaN never does.
__device__ __forceinline__ bool pr_better(double d, int i, double bd, int bi) {
    return d == d && i >= 0 && (bi < 0 || d < bd || (d == bd && i < bi));
}

// G = Sigma[cols, cols] for cols = {a0, a1, b0, b1}; -> the score, NaN when flagged; *flag as k_dsp_score's.
__device__ __forceinline__ double pair_score(const double (&G)[4][4], double r_merge, double nu0, double nu1, int* flag) {
    const double hc[2][4] = {{1.0, 0.0, -1.0, 0.0}, {0.0, 1.0, 0.0, -1.0}};
    const double R[2][2] = {{r_merge, 0.0}, {0.0, r_merge}};
    const double nan = __builtin_nan("");
    *flag = 1;
    double Tl[2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) acc = fma(hc[a][k], G[k][b], acc);
            Tl[a][b] = acc;
        }
    double M[2][4];   // [S | I]
    bool bad = false;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            double acc = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) acc = fma(Tl[a][k], hc[b][k], acc);
            const double val = acc + R[a][b];
            if (!isfinite(val)) bad = true;
            M[a][b] = val;
            M[a][2 + b] = a == b ? 1.0 : 0.0;
        }
    if (bad) return nan;
    {   // p = 0: rows 0 and 1 compete
        const bool low = fabs(M[1][0]) > fabs(M[0][0]);   // the pivot row is 1
        const double pv = low ? M[1][0] : M[0][0];
        if (!(fabs(pv) > 0.0)) return nan;
        double prow[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const double x = low ? M[1][c] : M[0][c], other = low ? M[0][c] : M[1][c];
            prow[c] = x / pv;
            M[0][c] = prow[c];
            M[1][c] = other;
        }
        const double f = M[1][0];
#pragma unroll
        for (int c = 1; c < 4; c++) M[1][c] = M[1][c] - f * prow[c];
    }
    {   // p = 1: row 1 alone
        const double pv = M[1][1];
        if (!isfinite(pv) || !(fabs(pv) > 0.0)) return nan;
        double prow[4];
#pragma unroll
        for (int c = 2; c < 4; c++) {
            prow[c] = M[1][c] / pv;
            M[1][c] = prow[c];
        }
        const double f = M[0][1];
#pragma unroll
        for (int c = 2; c < 4; c++) M[0][c] = M[0][c] - f * prow[c];
    }
    if (!isfinite(M[0][2]) || !isfinite(M[0][3]) || !isfinite(M[1][2]) || !isfinite(M[1][3])) return nan;
    *flag = 0;
    double w[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        double v = 0.0;
        v += M[t][2] * nu0;
        v += M[t][3] * nu1;
        w[t] = v;
    }
    double v = 0.0;
    v += nu0 * w[0];
    v += nu1 * w[1];
    return v;
}

// part_d2, part_idx: [tiles + 1][tiles * 32]; landmark tile T owns slots [0, tiles - T) (its rows of pair tiles (T, B),
// slot B - T) and [tiles - T, tiles] (its columns of pair tiles (A, T), slot tiles - T + A).  cnt: {below, flagged}.
__global__ __launch_bounds__(kThreads) void k_dpr_tile(const double* __restrict__ S, const double* __restrict__ x, int ld,
                                                       int n_lm, int tiles, double r_merge, double gate,
                                                       double* __restrict__ part_d2, int* __restrict__ part_idx,
                                                       unsigned long long* __restrict__ cnt) {
    __shared__ __attribute__((aligned(16))) double Qs[kTS * kLdq];
    __shared__ double res[kTL * kRes];
    __shared__ unsigned int sc[2];
    const int t = threadIdx.x;
    // the tile: blockIdx.x = B (B + 1) / 2 + A, A <= B
    const int k = blockIdx.x;
    int B = (int)((sqrt(8.0 * k + 1.0) - 1.0) * 0.5);
    while ((B + 1) * (B + 2) / 2 <= k) B++;
    while (B * (B + 1) / 2 > k) B--;
    const int A = k - B * (B + 1) / 2;
    const int lim = 3 + 2 * n_lm;
    if (t < 2) sc[t] = 0;

    // Sigma[3 + 64 B + rr][3 + 64 A + cc] on its way to LDS: wave w takes rows w, w + 4, ..
    const int cc = t & (kTS - 1), w = t / kTS;
    double v[kFill];
#pragma unroll
    for (int u = 0; u < kFill; u++) {
        const int row = 3 + kTS * B + w + (kThreads / kTS) * u, col = 3 + kTS * A + cc;
        v[u] = (row < lim && col < lim) ? S[(size_t)row * ld + col] : 0.0;
    }
    // this lane's pairs: b = 32 B + j for all of them, a = 32 A + ih + 8 q
    const int j = t & (kTL - 1), ih = t / kTL;
    const int b = kTL * B + j;
    const bool b_in = b < n_lm;
    pair8 Pab[kPer][2], Daa[kPer][2], xa[kPer];
    pair8 Dbb[2] = {pair8{0.0, 0.0}, pair8{0.0, 0.0}}, xb = pair8{0.0, 0.0};
    bool valid[kPer];
    if (b_in) {
        xb = *reinterpret_cast<const pair8*>(x + 3 + 2 * b);
#pragma unroll
        for (int r = 0; r < 2; r++) Dbb[r] = *reinterpret_cast<const pair8*>(S + (size_t)(3 + 2 * b + r) * ld + 3 + 2 * b);
    }
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        const int a = kTL * A + ih + (kThreads / kTL) * q;
        valid[q] = b_in && a < b;   // (a < b < n_lm; on a diagonal tile the upper triangle)
        xa[q] = pair8{0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 2; r++) Pab[q][r] = Daa[q][r] = pair8{0.0, 0.0};
        if (valid[q]) {
            xa[q] = *reinterpret_cast<const pair8*>(x + 3 + 2 * a);
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const double* row = S + (size_t)(3 + 2 * a + r) * ld;
                Pab[q][r] = *reinterpret_cast<const pair8*>(row + 3 + 2 * b);
                Daa[q][r] = *reinterpret_cast<const pair8*>(row + 3 + 2 * a);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < kFill; u++) Qs[(w + (kThreads / kTS) * u) * kLdq + cc] = v[u];
    __syncthreads();

    unsigned int below = 0, flagged = 0;
#pragma unroll
    for (int q = 0; q < kPer; q++) {
        const int i = ih + (kThreads / kTL) * q;
        double d = __builtin_nan("");
        if (valid[q]) {
            double G[4][4];
#pragma unroll
            for (int r = 0; r < 2; r++) {
                const pair16 ba = *reinterpret_cast<const pair16*>(&Qs[(2 * j + r) * kLdq + 2 * i]);   // Sigma[b_r][a_c]
                G[r][0] = Daa[q][r].x;     G[r][1] = Daa[q][r].y;
                G[r][2] = Pab[q][r].x;     G[r][3] = Pab[q][r].y;
                G[2 + r][0] = ba.x;        G[2 + r][1] = ba.y;
                G[2 + r][2] = Dbb[r].x;    G[2 + r][3] = Dbb[r].y;
            }
            int flag = 0;
            d = pair_score(G, r_merge, xa[q].x - xb.x, xa[q].y - xb.y, &flag);
            if (flag) flagged++;
            else if (d < gate) below++;
        }
        res[i * kRes + j] = d;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        below += __shfl_down(below, off);
        flagged += __shfl_down(flagged, off);
    }
    if ((t & 63) == 0) {
        if (below) atomicAdd(&sc[0], below);
        if (flagged) atomicAdd(&sc[1], flagged);
    }
    __syncthreads();
    if (t < 2 && sc[t]) atomicAdd(cnt + t, (unsigned long long)sc[t]);

    // the tile's rows (t < 32: landmark 32 A + t over its b) and columns (t < 64: landmark 32 B + t - 32 over its a)
    if (t < 2 * kTL) {
        const bool rows = t < kTL;
        const int l = t & (kTL - 1);
        const int lm = kTL * (rows ? A : B) + l;
        if (lm < n_lm) {
            const int other = kTL * (rows ? B : A), step = rows ? 1 : kRes, at = rows ? l * kRes : l;
            double bd = __builtin_huge_val();
            int bi = -1;
            for (int e = 0; e < kTL; e++) {
                const double d = res[at + e * step];
                if (pr_better(d, other + e, bd, bi)) bd = d, bi = other + e;
            }
            const int slot = rows ? B - A : tiles - B + A;
            const size_t o = (size_t)slot * (tiles * kTL) + lm;
            part_d2[o] = bd;
            part_idx[o] = bi;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_dpr_fold(const double* __restrict__ part_d2, const int* __restrict__ part_idx,
                                                       int n_lm, int tiles, int* __restrict__ nearest,
                                                       double* __restrict__ d2) {
    __shared__ double sd[kFoldGroups][kTL];
    __shared__ int si[kFoldGroups][kTL];
    const int t = threadIdx.x, l = t & (kTL - 1), g = t / kTL;
    const int lm = kTL * blockIdx.x + l;
    double bd = __builtin_huge_val();
    int bi = -1;
    for (int s = g; s <= tiles; s += kFoldGroups) {   // (a landmark beyond n_lm has no records: its result is not stored)
        const size_t o = (size_t)s * (tiles * kTL) + lm;
        const double d = lm < n_lm ? part_d2[o] : 0.0;
        const int i = lm < n_lm ? part_idx[o] : -1;
        if (pr_better(d, i, bd, bi)) bd = d, bi = i;
    }
    sd[g][l] = bd;
    si[g][l] = bi;
    __syncthreads();
    if (g == 0 && lm < n_lm) {
        for (int h = 1; h < kFoldGroups; h++)
            if (pr_better(sd[h][l], si[h][l], bd, bi)) bd = sd[h][l], bi = si[h][l];
        nearest[lm] = bi;
        d2[lm] = bi < 0 ? __builtin_huge_val() : bd;
    }
}

__global__ void k_dpr_terms(const double* __restrict__ x, int lo, int hi, double r_merge, int* __restrict__ cols,
                            double* __restrict__ Hc, double* __restrict__ R, double* __restrict__ nu) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int c[4] = {3 + 2 * lo, 4 + 2 * lo, 3 + 2 * hi, 4 + 2 * hi};
    const double h[8] = {1.0, 0.0, -1.0, 0.0, 0.0, 1.0, 0.0, -1.0};
    for (int k = 0; k < 4; k++) cols[k] = c[k];
    for (int k = 0; k < 8; k++) Hc[k] = h[k];
    R[0] = r_merge; R[1] = 0.0; R[2] = 0.0; R[3] = r_merge;
    nu[0] = x[c[2]] - x[c[0]];   // z - H x for the reading z = 0 of x_lo - x_hi: the scan's nu negated, exactly
    nu[1] = x[c[3]] - x[c[1]];
}

}  // namespace

Dense64PairsPlan dense64_pairs_plan(int n_lm) {
    Dense64PairsPlan p{};
    p.n_lm = n_lm;
    p.tiles = (n_lm + kTL - 1) / kTL;
    const size_t rec = (size_t)(p.tiles + 1) * p.tiles * kTL, out = (size_t)p.tiles * kTL;
    p.off_count = 0;                                   // two 64-bit words
    p.off_d2 = 16;                                     // [n_lm] doubles (room for tiles * 32)
    p.off_part_d2 = p.off_d2 + sizeof(double) * out;   // [tiles + 1][tiles * 32] doubles
    p.off_part_idx = p.off_part_d2 + sizeof(double) * rec;
    p.off_nearest = p.off_part_idx + sizeof(int) * rec;
    p.bytes = p.off_nearest + sizeof(int) * out;
    return p;
}

void launch_dense64_pairs(const Dense64PairsPlan& p, const double* Sigma, const double* state, int ld, double r_merge,
                          double gate, void* ws, hipStream_t st) {
    char* b = static_cast<char*>(ws);
    double* part_d2 = reinterpret_cast<double*>(b + p.off_part_d2);
    int* part_idx = reinterpret_cast<int*>(b + p.off_part_idx);
    hipLaunchKernelGGL(k_dpr_tile, dim3(p.tiles * (p.tiles + 1) / 2), dim3(kThreads), 0, st, Sigma, state, ld, p.n_lm,
                       p.tiles, r_merge, gate, part_d2, part_idx, reinterpret_cast<unsigned long long*>(b + p.off_count));
    hipLaunchKernelGGL(k_dpr_fold, dim3(p.tiles), dim3(kThreads), 0, st, part_d2, part_idx, p.n_lm, p.tiles,
                       reinterpret_cast<int*>(b + p.off_nearest), reinterpret_cast<double*>(b + p.off_d2));
}

void launch_dense64_pair_terms(const double* state, int lo, int hi, double r_merge, int* cols, double* Hc, double* R,
                               double* nu, hipStream_t st) {
    hipLaunchKernelGGL(k_dpr_terms, dim3(1), dim3(64), 0, st, state, lo, hi, r_merge, cols, Hc, R, nu);
}

}  // namespace ekf
