// ekf_dense64_factor.hip -- the Cholesky factor of the dense fp64 handle's live corner, Sigma[0:Na, 0:Na] = L L^T, and what
// is done against it: the forward substitution Y = L^-1 B, the backward substitution X = L^-T Y and the colouring product
// X = Z L^T (+ state) (gfx950, wave64).  The definitions are include/ekfslam.h's.  A blocked
// right-looking factorisation with block side NB = kDense64FactorNB = 64 in a snapshot buffer of the handle's own, so Sigma
// is only read.  The snapshot is `rows` x ldf, rows = Na rounded up to NB, ldf = rows + NB, zero wherever the corner is
// not: no tile of it is ragged, and the only masked accesses are those of Sigma itself (k_df_copy).
//   k_df_copy    a workgroup per NB x NB tile on or below the diagonal: Sigma[i][j], j <= i < Na, along rows into the
//                snapshot, 0.0 elsewhere in the tile.  Nothing of Sigma above the diagonal or at an index >= Na is read.
//   k_df_diag    ONE workgroup factors the diagonal block: the block lives in registers (16 entries a thread), column j goes
//                through LDS (two buffers: one barrier a column), every thread takes d_j, its square root and the quotients
//                it needs from there (correctly rounded sqrt and division, the same bits in every thread) and takes
//                l_ij l_kj out of its entries.  The first d_j that is not (finite and > 0) ends the call: the verdict word
//                is set and nothing of the block is stored.  One record per block: smallest / largest pivot, the failure.
//   k_df_panel   a wave per NB rows below the block, a thread per row: x L11^T = a by forward substitution, the row in
//                registers, L11 packed in LDS (every lane reads the same word), the tile in and out through LDS so that
//                global loads and stores run along rows.  Stores L21 in place and -L21 into the last NB columns.
//   k_df_update  a workgroup per NB x NB tile of the trailing lower triangle: gemm_tile<double, BT> of ekf_dense_gemm.hpp
//                (the 64 x 64 tile of the propagation's tail, v_mfma_f64_16x16x4_f64) with A = -L21, B = L21 and
//                C = Qadd = the tile itself: A22 <- A22 + (-L21) L21^T.  (An element of C is read and written by the same
//                lane and by no other, so C and Qadd may be the same memory.)  Tiles above the diagonal are not computed;
//                a diagonal tile is computed whole and its upper half lands in the snapshot's upper triangle, which
//                nothing reads.
//   k_dw_step    Y = L^-1 B, one launch per block column for all right-hand sides: a thread per right-hand side solves the
//                diagonal block (the substitution of k_df_panel); workgroup 0 stores Y's NB entries, workgroup g > 0 takes
//                L[rows of tile g, block] y out of its NB entries of the working copy, each wave a quarter of the rows.
//   k_dw_norm    d2[r] = sum_i Y[r][i]^2: strided partial sums and a binary fold in LDS.
//   k_ds_back    X = L^-T Y, the mirror of k_dw_step, one launch per block column, descending: a thread per right-hand side
//                solves L_bb^T x = y (descending, divisions by L[i][i]; columns >= Na are not divided); workgroup 0 stores
//                X's NB entries, workgroup g > 0 takes L[block b, block b - g]^T x_b out of its NB entries of the working
//                copy.  That tile is a row tile of L: it comes in along memory rows, and the transposition is the index of
//                the (broadcast) LDS read.
//   k_dc_color   X = Z L^T (+ state), ONE launch, a workgroup per NB states (the longest rows first).  The block columns
//                left of the diagonal are one gemm_tile<double, BT> with A = Z, B = the NB rows of L, K = NB * tile -- an
//                fp64 MFMA chain per element, ascending in k; the diagonal block continues each chain with plain
//                multiply-adds over k <= i out of the packed block, so nothing above the diagonal is taken from memory;
//                the state is added last.
// Every kernel of a block column starts with a read of the verdict word and returns on a failed pivot before its first
// store.  Three dependent launches per block column, no waits inside a kernel, no atomics at all: the order of every sum is
// a function of (Na, NB) alone and a run repeats bit for bit.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense_gemm.hpp"

namespace ekf {

namespace {

constexpr int kNB = kDense64FactorNB;
constexpr int kThreads = kDense64FactorThreads;
constexpr int kTs = kNB + 1;                    // LDS row stride of a transposed tile: odd, conflict-free 8-byte reads
constexpr int kPacked = kNB * (kNB + 1) / 2;    // a lower-triangular block, row i at i (i + 1) / 2
using UpdateTile = GemmTailTile<double, true>;
static_assert(kNB == 64 && kThreads == 256 && 128 % kNB == 0 && kNB >= 16, "a wave per block side, 16 entries a thread");
static_assert(UpdateTile::TM == kNB && UpdateTile::TN == kNB && kNB % UpdateTile::BK == 0, "the trailing tile is the block");

// the tile of a workgroup on or below the diagonal: k = B (B + 1) / 2 + A, A <= B
__device__ __forceinline__ void tile_pair(int k, int* A, int* B) {
    int b = (int)((sqrt(8.0 * k + 1.0) - 1.0) * 0.5);
    while ((b + 1) * (b + 2) / 2 <= k) b++;
    while (b * (b + 1) / 2 > k) b--;
    *B = b;
    *A = k - b * (b + 1) / 2;
}

__global__ __launch_bounds__(kThreads) void k_df_copy(const double* __restrict__ S, int ld, int Na, double* __restrict__ F,
                                                      int ldf) {
    int A, B;
    tile_pair(blockIdx.x, &A, &B);
    const int c = threadIdx.x & (kNB - 1), w = threadIdx.x / kNB;
    const int col = kNB * A + c;
#pragma unroll
    for (int u = 0; u < kNB / (kThreads / kNB); u++) {
        const int row = kNB * B + w + (kThreads / kNB) * u;
        F[(size_t)row * ldf + col] = (row < Na && col <= row) ? S[(size_t)row * ld + col] : 0.0;
    }
}

// x <- L^-1 x for the packed lower-triangular block Lp (LDS), ascending; entries from nb on become 0.0
__device__ __forceinline__ void forward_substitute(const double* Lp, double (&x)[kNB], int nb) {
#pragma unroll
    for (int j = 0; j < kNB; j++) {
        const double* row = Lp + j * (j + 1) / 2;
        double s = x[j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= x[k] * row[k];
        x[j] = j < nb ? s / row[j] : 0.0;
    }
}

// x <- L^-T x for the packed block, descending; entries from nb on are not divided: they become 0.0
__device__ __forceinline__ void backward_substitute(const double* Lp, double (&x)[kNB], int nb) {
#pragma unroll
    for (int j = kNB - 1; j >= 0; j--) {
        double s = x[j];
#pragma unroll
        for (int k = kNB - 1; k > j; k--) s -= Lp[k * (k + 1) / 2 + j] * x[k];
        x[j] = j < nb ? s / Lp[j * (j + 1) / 2 + j] : 0.0;
    }
}

__device__ __forceinline__ void load_packed(const double* __restrict__ Fb, int ldf, double* Lp, int t, int nthreads) {
    for (int e = t; e < kNB * kNB; e += nthreads) {
        const int i = e / kNB, k = e % kNB;
        if (k <= i) Lp[i * (i + 1) / 2 + k] = Fb[(size_t)i * ldf + k];
    }
}

__global__ __launch_bounds__(kThreads) void k_df_diag(double* __restrict__ F, int ldf, int Na, int b, int* __restrict__ verdict,
                                                      Dense64FactorRecord* __restrict__ rec, double* __restrict__ diag) {
    __shared__ double cbuf[2][kNB];
    __shared__ double sdiag[kNB];
    if (*verdict) return;
    const int t = threadIdx.x, ti = t >> 4, tk = t & 15;
    const int j0 = kNB * b, nb = min(kNB, Na - j0);
    double* Fb = F + (size_t)j0 * ldf + j0;
    double v[4][4];   // entry (i = ti + 16 a, k = tk + 16 c) of the block
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int i = ti + 16 * a, k = tk + 16 * c;
            v[a][c] = k <= i ? Fb[(size_t)i * ldf + k] : 0.0;
        }
    double mn = __builtin_huge_val(), mx = 0.0, fail_pivot = 0.0;
    int mn_i = -1, fail = -1;
    for (int j = 0; j < nb; j++) {
        double* cb = cbuf[j & 1];
        if (tk == (j & 15)) {   // the owners of column j hand it on as it stands
            const int cq = j >> 4;
#pragma unroll
            for (int a = 0; a < 4; a++) {
                double val = v[a][0];
#pragma unroll
                for (int c = 1; c < 4; c++) val = c == cq ? v[a][c] : val;
                cb[ti + 16 * a] = val;
            }
        }
        __syncthreads();
        const double d = cb[j];
        if (!(d > 0.0 && d < __builtin_huge_val())) {   // (the same word in every thread)
            fail = j0 + j;
            fail_pivot = d;
            break;
        }
        if (d < mn) mn = d, mn_i = j0 + j;
        if (d > mx) mx = d;
        const double l = sqrt(d);
        if (t == 0) sdiag[j] = l;
        double li[4], lk[4];
#pragma unroll
        for (int a = 0; a < 4; a++) li[a] = cb[ti + 16 * a] / l;
#pragma unroll
        for (int c = 0; c < 4; c++) lk[c] = cb[tk + 16 * c] / l;
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int i = ti + 16 * a, k = tk + 16 * c;
                if (k == j) v[a][c] = i > j ? li[a] : (i == j ? l : v[a][c]);
                else if (k > j && i >= k) v[a][c] -= li[a] * lk[c];
            }
    }
    if (t == 0) {
        rec[b].min_pivot = mn, rec[b].max_pivot = mx, rec[b].min_i = mn_i;
        rec[b].fail_pivot = fail_pivot, rec[b].fail_index = fail;
        if (fail >= 0) *verdict = 1;
    }
    if (fail >= 0) return;
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int i = ti + 16 * a, k = tk + 16 * c;
            if (k <= i && i < nb) Fb[(size_t)i * ldf + k] = v[a][c];
        }
    if (t < nb) diag[j0 + t] = sdiag[t];
}

// rows [c0 + NB g, + NB) of block column b, c0 = NB (b + 1); `rows` = where the negated panel goes
__global__ __launch_bounds__(kNB) void k_df_panel(double* __restrict__ F, int ldf, int rows, int b,
                                                  const int* __restrict__ verdict) {
    __shared__ double Lp[kPacked];
    __shared__ double tile[kNB * kTs];
    if (*verdict) return;
    const int t = threadIdx.x, j0 = kNB * b;
    const int r0 = j0 + kNB * (1 + blockIdx.x);
    load_packed(F + (size_t)j0 * ldf + j0, ldf, Lp, t, kNB);
    double* Fr = F + (size_t)r0 * ldf;
    for (int r = 0; r < kNB; r++) tile[r * kTs + t] = Fr[(size_t)r * ldf + j0 + t];
    __syncthreads();
    double x[kNB];
#pragma unroll
    for (int j = 0; j < kNB; j++) x[j] = tile[t * kTs + j];
    forward_substitute(Lp, x, kNB);
#pragma unroll
    for (int j = 0; j < kNB; j++) tile[t * kTs + j] = x[j];
    __syncthreads();
    for (int r = 0; r < kNB; r++) {
        const double val = tile[r * kTs + t];
        Fr[(size_t)r * ldf + j0 + t] = val;
        Fr[(size_t)r * ldf + rows + t] = -val;
    }
}

__global__ __launch_bounds__(kThreads, 4) void k_df_update(double* F, int ldf, int rows, int b, const int* __restrict__ verdict) {
    extern __shared__ __attribute__((aligned(16))) unsigned char df_smem[];
    if (*verdict) return;
    int tn, tm;
    tile_pair(blockIdx.x, &tn, &tm);
    const int c0 = kNB * (b + 1);
    gemm_tile<double, true, UpdateTile::NBUF, UpdateTile::WTM, UpdateTile::WTN>(
        F + rows, F + kNB * b, F, F, ldf, c0 + kNB * tm, c0 + kNB * tn, reinterpret_cast<double*>(df_smem), kNB);
}

// block column b of the substitution; workgroup g: the tile of rows NB (b + g)
__global__ __launch_bounds__(kThreads) void k_dw_step(const double* __restrict__ F, int ldf, int Na, int rows, int b,
                                                      double* __restrict__ work, double* __restrict__ Y) {
    __shared__ double Lp[kPacked];
    __shared__ double Lt[kNB * kNB];
    const int t = threadIdx.x, r = t & (kNB - 1), w = t / kNB;
    const int j0 = kNB * b, nb = min(kNB, Na - j0), g = blockIdx.x;
    const int i0 = j0 + kNB * g;
    load_packed(F + (size_t)j0 * ldf + j0, ldf, Lp, t, kThreads);
    if (g > 0)
        for (int e = t; e < kNB * kNB; e += kThreads) Lt[e] = F[(size_t)(i0 + e / kNB) * ldf + j0 + e % kNB];
    double y[kNB];
    const double* src = work + (size_t)r * rows + j0;
#pragma unroll
    for (int j = 0; j < kNB; j++) y[j] = src[j];
    __syncthreads();
    forward_substitute(Lp, y, nb);
    if (g == 0) {
        if (w == 0) {
            double* dst = Y + (size_t)r * rows + j0;
#pragma unroll
            for (int j = 0; j < kNB; j++) dst[j] = y[j];
        }
        return;
    }
    constexpr int kPerWave = kNB / (kThreads / kNB);
    double* mine = work + (size_t)r * rows + i0 + kPerWave * w;
    for (int u = 0; u < kPerWave; u++) {
        const double* row = Lt + (kPerWave * w + u) * kNB;
        double s = mine[u];
#pragma unroll
        for (int k = 0; k < kNB; k++) s -= row[k] * y[k];
        mine[u] = s;
    }
}

__global__ __launch_bounds__(kThreads) void k_dw_norm(const double* __restrict__ Y, int rows, double* __restrict__ d2) {
    __shared__ double part[kThreads];
    const int t = threadIdx.x;
    const double* y = Y + (size_t)blockIdx.x * rows;
    double s = 0.0;
    for (int i = t; i < rows; i += kThreads) s += y[i] * y[i];
    part[t] = s;
    __syncthreads();
    for (int half = kThreads / 2; half > 0; half >>= 1) {
        if (t < half) part[t] += part[t + half];
        __syncthreads();
    }
    if (t == 0) d2[blockIdx.x] = part[0];
}

// block column b of the backward substitution; workgroup g: the tile of columns NB (b - g), 0 <= g <= b
__global__ __launch_bounds__(kThreads) void k_ds_back(const double* __restrict__ F, int ldf, int Na, int rows, int b,
                                                      double* __restrict__ work, double* __restrict__ X) {
    __shared__ double Lp[kPacked];
    __shared__ double Lt[kNB * kNB];
    const int t = threadIdx.x, r = t & (kNB - 1), w = t / kNB;
    const int j0 = kNB * b, nb = min(kNB, Na - j0), g = blockIdx.x;
    const int c0 = j0 - kNB * g;
    load_packed(F + (size_t)j0 * ldf + j0, ldf, Lp, t, kThreads);
    if (g > 0)   // L[j0 + i][c0 + k] at Lt[i][k]: rows of the snapshot
        for (int e = t; e < kNB * kNB; e += kThreads) Lt[e] = F[(size_t)(j0 + e / kNB) * ldf + c0 + e % kNB];
    double x[kNB];
    const double* src = work + (size_t)r * rows + j0;
#pragma unroll
    for (int j = 0; j < kNB; j++) x[j] = src[j];
    __syncthreads();
    backward_substitute(Lp, x, nb);
    if (g == 0) {
        if (w == 0) {
            double* dst = X + (size_t)r * rows + j0;
#pragma unroll
            for (int j = 0; j < kNB; j++) dst[j] = x[j];
        }
        return;
    }
    constexpr int kPerWave = kNB / (kThreads / kNB);
    double* mine = work + (size_t)r * rows + c0 + kPerWave * w;
    for (int u = 0; u < kPerWave; u++) {
        const double* col = Lt + kPerWave * w + u;
        double s = mine[u];
#pragma unroll
        for (int i = 0; i < kNB; i++) s -= col[i * kNB] * x[i];
        mine[u] = s;
    }
}

constexpr size_t kColorLdsBytes = UpdateTile::kLdsBytes + sizeof(double) * kPacked;   // the GEMM tile's image | the packed block
static_assert(UpdateTile::kLdsBytes % 16 == 0, "the packed block sits on a 16-byte boundary of the dynamic region");

// row tile `tile` of X = Z L^T: Z and X are [kNB right-hand sides][ldf], the snapshot's own row stride
__global__ __launch_bounds__(kThreads) void k_dc_color(const double* __restrict__ F, int ldf, int Na, int blocks,
                                                       const double* __restrict__ Z, const double* __restrict__ state,
                                                       double* X) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dc_smem[];
    double* Lp = reinterpret_cast<double*>(dc_smem + UpdateTile::kLdsBytes);
    const int tile = blocks - 1 - (int)blockIdx.x;   // the longest rows start first
    const int t = threadIdx.x, r = t & (kNB - 1);
    const int w = __builtin_amdgcn_readfirstlane(t / kNB);
    const int j0 = kNB * tile;
    load_packed(F + (size_t)j0 * ldf + j0, ldf, Lp, t, kThreads);
    if (tile > 0)   // X[:, tile] = Z[:, 0 : j0] L[tile rows, 0 : j0]^T
        gemm_tile<double, true, UpdateTile::NBUF, UpdateTile::WTM, UpdateTile::WTN>(Z, F, X, nullptr, ldf, 0, j0,
                                                                                   reinterpret_cast<double*>(dc_smem), j0);
    __syncthreads();   // Lp, and the tile of X that other lanes wrote
    double z[kNB];
    const double* src = Z + (size_t)r * ldf + j0;
#pragma unroll
    for (int k = 0; k < kNB; k++) z[k] = src[k];
    constexpr int kPerWave = kNB / (kThreads / kNB);
    double* mine = X + (size_t)r * ldf + j0 + kPerWave * w;
    for (int u = 0; u < kPerWave; u++) {
        const int i = kPerWave * w + u;   // (the same in every lane of a wave)
        const double* row = Lp + i * (i + 1) / 2;
        double s = tile > 0 ? mine[u] : 0.0;
#pragma unroll
        for (int k = 0; k < kNB; k++)
            if (k <= i) s += row[k] * z[k];
        if (state && j0 + i < Na) s += state[j0 + i];
        mine[u] = s;
    }
}

}  // namespace

Dense64FactorPlan dense64_factor_plan(int Na) {
    Dense64FactorPlan p{};
    p.Na = Na;
    p.blocks = (Na + kNB - 1) / kNB;
    p.rows = p.blocks * kNB;
    p.ldf = p.rows + kNB;
    p.factor_bytes = sizeof(double) * (size_t)p.rows * p.ldf;
    p.off_verdict = 0;
    p.off_rec = 16;
    p.off_diag = p.off_rec + sizeof(Dense64FactorRecord) * (size_t)p.blocks;
    p.bytes = p.off_diag + sizeof(double) * (size_t)p.rows;
    return p;
}

void launch_dense64_factor(const Dense64FactorPlan& p, const double* Sigma, int ld, double* factor, void* ws, hipStream_t st) {
    char* base = static_cast<char*>(ws);
    int* verdict = reinterpret_cast<int*>(base + p.off_verdict);
    Dense64FactorRecord* rec = reinterpret_cast<Dense64FactorRecord*>(base + p.off_rec);
    double* diag = reinterpret_cast<double*>(base + p.off_diag);
    const unsigned lower = (unsigned)((size_t)p.blocks * (p.blocks + 1) / 2);
    hipLaunchKernelGGL(k_df_copy, dim3(lower), dim3(kThreads), 0, st, Sigma, ld, p.Na, factor, p.ldf);
    for (int b = 0; b < p.blocks; b++) {
        hipLaunchKernelGGL(k_df_diag, dim3(1), dim3(kThreads), 0, st, factor, p.ldf, p.Na, b, verdict, rec, diag);
        const int below = p.blocks - 1 - b;   // tiles of NB rows under the block
        if (below == 0) break;
        hipLaunchKernelGGL(k_df_panel, dim3(below), dim3(kNB), 0, st, factor, p.ldf, p.rows, b, verdict);
        hipLaunchKernelGGL(k_df_update, dim3((unsigned)((size_t)below * (below + 1) / 2)), dim3(kThreads),
                           UpdateTile::kLdsBytes, st, factor, p.ldf, p.rows, b, verdict);
    }
}

void launch_dense64_whiten(const Dense64FactorPlan& p, const double* factor, double* rhs, double* d2, hipStream_t st) {
    double* Y = rhs + (size_t)kDense64WhitenMaxRhs * p.rows;
    for (int b = 0; b < p.blocks; b++)
        hipLaunchKernelGGL(k_dw_step, dim3(p.blocks - b), dim3(kThreads), 0, st, factor, p.ldf, p.Na, p.rows, b, rhs, Y);
    hipLaunchKernelGGL(k_dw_norm, dim3(kDense64WhitenMaxRhs), dim3(kThreads), 0, st, Y, p.rows, d2);
}

void launch_dense64_back(const Dense64FactorPlan& p, const double* factor, double* work, double* X, hipStream_t st) {
    for (int b = p.blocks - 1; b >= 0; b--)
        hipLaunchKernelGGL(k_ds_back, dim3(b + 1), dim3(kThreads), 0, st, factor, p.ldf, p.Na, p.rows, b, work, X);
}

void launch_dense64_color(const Dense64FactorPlan& p, const double* factor, const double* Z, const double* state, double* X,
                          hipStream_t st) {
    hipLaunchKernelGGL(k_dc_color, dim3(p.blocks), dim3(kThreads), kColorLdsBytes, st, factor, p.ldf, p.Na, p.blocks, Z,
                       state, X);
}

}  // namespace ekf
