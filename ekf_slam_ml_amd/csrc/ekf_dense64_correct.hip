// ekf_dense64_correct.hip -- dense fp64 measurement update for an ARBITRARY m x N Jacobian H (1 <= m <= 64), the other half
// of the dense family: the reference's literal correction (rigid2d/src/ekf_slam.cpp:178,186,191-192)
//   Ki = sigma*Hj.t()*(Hj*sigma*Hj.t() + R).i();   state = state + Ki*z_diff;   sigma = (eye(size(kh)) - kh)*sigma
// for general operands, streamed as
//   T = H Sigma (rows of Sigma)   U = Sigma H^T (COLUMNS of Sigma: Sigma is never symmetrised)
//   S = T H^T + R   K = U S^-1   state += K nu   Sigma <- Sigma - K T   nis = nu^T S^-1 nu
// Memory-bound work (6 m N^2 flop over >= 24 N^2 bytes), six launches on one stream, no floating-point atomics anywhere:
// every sum has a fixed order, so a correction is bit-identical from run to run.
//   1 k_dc_panels   ONE pass over Sigma.  A workgroup walks a super-tile (a chunk of 64-row tiles x a strip of up to four
//                   64-column tiles); each 64 x 64 tile goes global -> registers -> LDS once and feeds both panels from
//                   there on v_mfma_f64_16x16x4_f64: T[:, J] += H[:, I] Sigma[I, J] (B operand read along rows) and
//                   U[I, :]^T += H[:, J] Sigma[I, J]^T (B operand read along columns).  T accumulates in registers over the
//                   chunk's row tiles, U over the strip's column tiles; what is left are partial panels per row chunk (T)
//                   and per strip (U).
//   2 k_dc_sum      partial panels summed in index order -> T [m][ld], U^T [m][ld] (entries >= N written as zeros)
//   3 k_dc_spart    per 128-column chunk: T[:, chunk] H[:, chunk]^T (m x m)
//   4 k_dc_invert   one workgroup: S = (sum of the chunks, in order) + R, Gauss-Jordan with partial pivoting in LDS (the
//                   routine of ekf_dense64_invert.hpp, shared with the candidate scoring of ekf_dense64_score.hip), the
//                   verdict (zero / non-finite pivot, non-finite S or S^-1) into a device word, S^-1, nis
//   5 k_dc_gain     K = U S^-1 (stored as K^T [m][ld]), state += K nu
//   6 k_dc_update   Sigma <- Sigma - K T in place on v_mfma_f64_16x16x4_f64: the Sigma tile is the accumulator, -K comes
//                   from the (cache-resident) K^T panel, T from LDS, k = m rounded up to 4 with zero fill
// Launches 5 and 6 read the verdict on the device and return before their first write when it is set, so state and Sigma
// stay exactly as they were and the host needs one synchronisation per correction, not two.
// Lane maps of v_mfma_f64_16x16x4_f64 (as GemmTraits<double> in ekf_dense_gemm.hpp): A: lane l holds A[i = l & 15][k = l >> 4];
// B: B[k = l >> 4][j = l & 15]; C/D: col = l & 15, row = (l >> 4) + 4 * reg.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense_gemm.hpp"   // f64x4, f64x2, GemmTraits<double>::mfma
#include "ekf_dense64_invert.hpp"

namespace ekf {

namespace {

constexpr int kMaxM = kDense64MaxM;   // 64: row stride of every panel and of the m x m matrices
constexpr int kTile = 64;             // Sigma tile of the panel pass
constexpr int kTileS = kTile + 2;     // LDS row stride: 2 (mod 32) doubles -> the column-wise B reads hit 64 distinct banks
constexpr int kStripTiles = 4;        // column tiles per super-tile (strip = 256 columns)
constexpr int kUpdCols = 128;         // column strip of the rank-m update
constexpr int kGainRows = 32;         // rows of K per workgroup of the gain kernel

// ---- 1: panels --------------------------------------------------------------------------------------------------------
// Ht: H transposed, [ld][16 MB] (k contiguous; MB = m rounded up to 16, in sixteens), zero for k >= m and for rows >= N.
// Tpart [n_chunks][64][ld], Upart [n_strips][64][ld] (rows k < 16 * MB of each are written where the tiles are real).
template <int MB>
__global__ __launch_bounds__(256) void k_dc_panels(const double* __restrict__ S, const double* __restrict__ Ht,
                                                   double* __restrict__ Tpart, double* __restrict__ Upart, int N, int ld,
                                                   int tiles_per_chunk) {
    constexpr int HS = 16 * MB + 2;   // LDS row stride of the H tiles
    extern __shared__ __attribute__((aligned(16))) double dc_smem[];
    double* tile = dc_smem;                     // [64][kTileS]
    double* hr = tile + kTile * kTileS;         // [64 rows i of the tile][16 MB]  = H[:, I]^T
    double* hc = hr + kTile * HS;               // [64 cols j of the tile][16 MB]  = H[:, J]^T

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int strip = blockIdx.x, chunk = blockIdx.y;
    const int col_base = strip * kStripTiles * kTile;
    const int n_row_tiles = (N + kTile - 1) / kTile;
    const int rt0 = chunk * tiles_per_chunk;
    const int rt1 = min(n_row_tiles, rt0 + tiles_per_chunk);
    int nct = (N - col_base + kTile - 1) / kTile;   // column tiles of this strip that hold real columns
    if (nct > kStripTiles) nct = kStripTiles;
    if (rt0 >= rt1 || nct <= 0) return;   // (uniform; the host launches no such workgroup)

    f64x2 pre[8];
    auto gload = [&](int rt, int ct) {
        const double* g = S + (size_t)(rt * kTile) * ld + col_base + ct * kTile;
#pragma unroll
        for (int p = 0; p < 8; p++)
            pre[p] = *reinterpret_cast<const f64x2*>(g + (size_t)((t >> 5) + 8 * p) * ld + (t & 31) * 2);
    };
    auto hload = [&](double* dst, int first) {   // 64 rows of Ht starting at `first`
        for (int e = t; e < kTile * MB * 8; e += 256) {
            const int row = e / (MB * 8), c2 = (e % (MB * 8)) * 2;
            *reinterpret_cast<f64x2*>(dst + row * HS + c2) =
                *reinterpret_cast<const f64x2*>(Ht + (size_t)(first + row) * (16 * MB) + c2);
        }
    };

    f64x4 accT[kStripTiles][MB], accU[MB];
#pragma unroll
    for (int c = 0; c < kStripTiles; c++)
#pragma unroll
        for (int b = 0; b < MB; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) accT[c][b][r] = 0.0;

    gload(rt0, 0);
    for (int rt = rt0; rt < rt1; rt++) {
#pragma unroll
        for (int b = 0; b < MB; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) accU[b][r] = 0.0;
#pragma unroll
        for (int ct = 0; ct < kStripTiles; ct++) {
            if (ct < nct) {   // (uniform)
                __syncthreads();   // every wave is done reading the previous tile
#pragma unroll
                for (int p = 0; p < 8; p++)
                    *reinterpret_cast<f64x2*>(tile + ((t >> 5) + 8 * p) * kTileS + (t & 31) * 2) = pre[p];
                if (ct == 0) hload(hr, rt * kTile);
                hload(hc, col_base + ct * kTile);
                __syncthreads();
                // the next tile's global loads fly under this tile's MFMAs
                if (ct + 1 < nct) gload(rt, ct + 1);
                else if (rt + 1 < rt1) gload(rt + 1, 0);
                // T[k][j] += H[k][i] Sigma[i][j]: wave w owns the 16 columns j = 16 w + (0..15) of the tile
#pragma unroll 4
                for (int s = 0; s < kTile / 4; s++) {
                    const double b = tile[(4 * s + lk) * kTileS + 16 * w + li];
#pragma unroll
                    for (int kb = 0; kb < MB; kb++)
                        accT[ct][kb] = GemmTraits<double>::mfma(hr[(4 * s + lk) * HS + 16 * kb + li], b, accT[ct][kb]);
                }
                // U^T[k][i] += H[k][j] Sigma[i][j]: wave w owns the 16 rows i = 16 w + (0..15) of the tile
#pragma unroll 4
                for (int s = 0; s < kTile / 4; s++) {
                    const double b = tile[(16 * w + li) * kTileS + 4 * s + lk];
#pragma unroll
                    for (int kb = 0; kb < MB; kb++)
                        accU[kb] = GemmTraits<double>::mfma(hc[(4 * s + lk) * HS + 16 * kb + li], b, accU[kb]);
                }
            }
        }
        double* up = Upart + (size_t)strip * kMaxM * ld + rt * kTile + 16 * w + li;
#pragma unroll
        for (int kb = 0; kb < MB; kb++)
#pragma unroll
            for (int r = 0; r < 4; r++) up[(size_t)(16 * kb + lk + 4 * r) * ld] = accU[kb][r];
    }
    double* tp = Tpart + (size_t)chunk * kMaxM * ld + col_base + 16 * w + li;
#pragma unroll
    for (int ct = 0; ct < kStripTiles; ct++)
        if (ct < nct)
#pragma unroll
            for (int kb = 0; kb < MB; kb++)
#pragma unroll
                for (int r = 0; r < 4; r++) tp[(size_t)(16 * kb + lk + 4 * r) * ld + ct * kTile] = accT[ct][kb][r];
}

// ---- 2: partial panels -> panels, summed in index order; one thread per (k, pair of columns) ---------------------------
__global__ __launch_bounds__(256) void k_dc_sum(const double* __restrict__ Tpart, const double* __restrict__ Upart,
                                                double* __restrict__ Tp, double* __restrict__ Ut, int N, int ld, int m,
                                                int n_chunks, int n_strips) {
    const int j = (blockIdx.x * 256 + threadIdx.x) * 2;
    const int k = blockIdx.y;
    if (j >= ld || k >= m) return;
    f64x2 tv = {0.0, 0.0}, uv = {0.0, 0.0};
    if (j < N) {   // (beyond N the partial panels were never written)
        const size_t step = (size_t)kMaxM * ld;
        const double* p = Tpart + (size_t)k * ld + j;
        for (int c = 0; c < n_chunks; c++) tv += *reinterpret_cast<const f64x2*>(p + c * step);
        const double* q = Upart + (size_t)k * ld + j;
        for (int s = 0; s < n_strips; s++) uv += *reinterpret_cast<const f64x2*>(q + s * step);
        if (j + 1 >= N) tv[1] = 0.0, uv[1] = 0.0;   // the panels' padding is zero whatever Sigma's padding held
    }
    *reinterpret_cast<f64x2*>(Tp + (size_t)k * ld + j) = tv;
    *reinterpret_cast<f64x2*>(Ut + (size_t)k * ld + j) = uv;
}

// ---- 3: Spart[chunk][k][l] = sum over the chunk's 128 columns j (ascending) of T[k][j] H[l][j] ---------------------------
__global__ __launch_bounds__(256) void k_dc_spart(const double* __restrict__ Tp, const double* __restrict__ Hd,
                                                  double* __restrict__ Spart, int ld, int m) {
    __shared__ double tl[kMaxM][33], hl[kMaxM][33];
    const int t = threadIdx.x;
    double acc[16];
#pragma unroll
    for (int q = 0; q < 16; q++) acc[q] = 0.0;
    for (int sub = 0; sub < 4; sub++) {
        const int j0 = blockIdx.x * 128 + sub * 32;
        for (int e = t; e < m * 32; e += 256) {
            const int k = e >> 5, jj = e & 31;
            tl[k][jj] = Tp[(size_t)k * ld + j0 + jj];
            hl[k][jj] = Hd[(size_t)k * ld + j0 + jj];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const int o = t + 256 * q, k = o >> 6, l = o & 63;
            if (k < m && l < m)
                for (int jj = 0; jj < 32; jj++) acc[q] += tl[k][jj] * hl[l][jj];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int o = t + 256 * q, k = o >> 6, l = o & 63;
        if (k < m && l < m) Spart[(size_t)blockIdx.x * kMaxM * kMaxM + o] = acc[q];
    }
}

// ---- 4: S, its inverse, the verdict, nis -----------------------------------------------------------------------------
// out: Sinv [64][64] (stride 64), verdict[0] = 0 fine / 1 singular or non-finite, nis[0].
constexpr int kInvS = 2 * kMaxM + 1;   // row stride of the augmented matrix [S | I] in LDS

__global__ __launch_bounds__(256) void k_dc_invert(const double* __restrict__ Spart, int n_parts,
                                                   const double* __restrict__ R, const double* __restrict__ nu,
                                                   double* __restrict__ Sinv, double* __restrict__ nis,
                                                   int* __restrict__ verdict, int m) {
    extern __shared__ __attribute__((aligned(16))) double dc_smem[];
    double* M = dc_smem;                    // [m][kInvS]
    __shared__ int s_ctl[2];
    __shared__ double s_pv;
    // [2 m] the scaled pivot row | [m] the column being eliminated | [m] S^-1 nu
    const GjScratch sc{M + kMaxM * kInvS, M + kMaxM * kInvS + 2 * kMaxM, M + kMaxM * kInvS + 3 * kMaxM, &s_pv, s_ctl};
    const int t = threadIdx.x;
    int bad = 0;
    for (int e = t; e < m * m; e += 256) {
        const int k = e / m, l = e % m;
        double v = 0.0;
        for (int c = 0; c < n_parts; c++) v += Spart[(size_t)c * kMaxM * kMaxM + k * kMaxM + l];
        v += R[k * m + l];
        if (!isfinite(v)) bad = 1;
        M[k * kInvS + l] = v;
        M[k * kInvS + m + l] = k == l ? 1.0 : 0.0;
    }
    if (gj_invert<256>(M, kInvS, sc, m, t, bad)) {   // (uniform) the elimination of ekf_dense64_invert.hpp
        if (t == 0) verdict[0] = 1;
        return;
    }
    for (int e = t; e < m * m; e += 256) Sinv[(e / m) * kMaxM + e % m] = M[(e / m) * kInvS + m + e % m];
    if (nu) {   // nis = nu^T S^-1 nu, the score of calculate_maha_dis (:267-269)
        const double v = gj_quadratic<256>(M, kInvS, sc, m, t, nu);
        if (t == 0) nis[0] = v;
    }
    if (t == 0) verdict[0] = 0;
}

// ---- 5: K^T[k][i] = sum_l U^T[l][i] Sinv[l][k] (l ascending), state[i] += sum_k K[i][k] nu[k] ---------------------------
__global__ __launch_bounds__(256) void k_dc_gain(const double* __restrict__ Ut, const double* __restrict__ Sinv,
                                                 const double* __restrict__ nu, double* __restrict__ Kt,
                                                 double* __restrict__ state, const int* __restrict__ verdict, int N, int ld,
                                                 int m) {
    __shared__ double si[kMaxM][kMaxM], ul[kMaxM][kGainRows], sp[8][kGainRows];
    if (verdict[0] != 0) return;   // (uniform) the decision precedes every write
    const int t = threadIdx.x, i = t & (kGainRows - 1), g = t / kGainRows;   // g: 8 groups, k = g + 8 q
    const int i0 = blockIdx.x * kGainRows;
    for (int e = t; e < kMaxM * kMaxM; e += 256) {
        const int l = e >> 6, k = e & 63;
        si[l][k] = (l < m && k < m) ? Sinv[e] : 0.0;
    }
    for (int e = t; e < m * kGainRows; e += 256)
        ul[e / kGainRows][e % kGainRows] = Ut[(size_t)(e / kGainRows) * ld + i0 + e % kGainRows];
    __syncthreads();
    double acc[8];
#pragma unroll
    for (int q = 0; q < 8; q++) acc[q] = 0.0;
    for (int l = 0; l < m; l++) {
        const double u = ul[l][i];
#pragma unroll
        for (int q = 0; q < 8; q++) acc[q] += u * si[l][g + 8 * q];
    }
    const bool real = i0 + i < N;
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int k = g + 8 * q;
        if (k < m) {
            const double v = real ? acc[q] : 0.0;   // K's padding is zero whatever U's held
            Kt[(size_t)k * ld + i0 + i] = v;
            if (nu) part += v * nu[k];
        }
    }
    if (nu) {
        sp[g][i] = part;
        __syncthreads();
        if (g == 0 && real) {
            double v = sp[0][i];
#pragma unroll
            for (int q = 1; q < 8; q++) v += sp[q][i];
            state[i0 + i] = state[i0 + i] + v;
        }
    }
}

// ---- 6: Sigma <- Sigma - K T ---------------------------------------------------------------------------------------------
// Workgroup = a strip of 128 columns (its T panel sits in LDS) x a chunk of 16-row blocks dealt to the 4 waves.  A wave's
// unit is 16 rows x 128 columns = 4 column groups of 32, each two accumulators: lane (lk, li) owns the ADJACENT columns
// 32 g + 2 li, + 1 (one 16-byte access; a row of a group is 256 contiguous bytes), which the two MFMAs of the group see as
// their column li -- the B operand is read from LDS with the same pairing, so the permutation never shows.
// LIVE (the handle's live dimension N is smaller than its capacity, ekf_dense64_set_live): rows and columns >= N of Sigma are
// not padding but entries of the tail that the call must neither read nor write, so every load and store of the tile is
// masked by row < N and column < N (a pair that straddles N as its first element alone); a masked entry enters the MFMA as
// +0 and its result is dropped.  Row i of the product depends on row i of K and column j on column j of T alone, so what K^T
// and T hold at indices >= N (the leftovers of a wider call) reaches no stored entry.  LIVE = false is the kernel as it was.
template <bool LIVE>
__global__ __launch_bounds__(256) void k_dc_update(double* __restrict__ S, const double* __restrict__ Kt,
                                                   const double* __restrict__ Tp, const int* __restrict__ verdict, int N,
                                                   int ld, int m, int blocks_per_chunk) {
    extern __shared__ __attribute__((aligned(16))) double dc_smem[];   // [kp][128]
    if (verdict[0] != 0) return;   // (uniform) the decision precedes every write
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int kp = (m + 3) & ~3;
    const int c0 = blockIdx.x * kUpdCols;
    for (int e = t; e < kp * (kUpdCols / 2); e += 256) {
        const int k = e / (kUpdCols / 2), c2 = (e % (kUpdCols / 2)) * 2;
        f64x2 v = {0.0, 0.0};
        if (k < m) v = *reinterpret_cast<const f64x2*>(Tp + (size_t)k * ld + c0 + c2);
        if constexpr (LIVE) {   // (the panel is allocated up to ld; what it holds from N on is not this call's)
            if (c0 + c2 >= N) v[0] = 0.0;
            if (c0 + c2 + 1 >= N) v[1] = 0.0;
        }
        *reinterpret_cast<f64x2*>(dc_smem + k * kUpdCols + c2) = v;
    }
    __syncthreads();
    const int nb = (N + 15) / 16;
    const int b0 = blockIdx.y * blocks_per_chunk;
    const int b1 = min(nb, b0 + blocks_per_chunk);

    f64x2 cur[4][4], nxt[4][4];
    auto gload = [&](int b, f64x2 (&v)[4][4]) {
        const double* base = S + (size_t)(b * 16 + lk) * ld + c0 + 2 * li;
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double* src = base + (size_t)(4 * r) * ld + 32 * g;
                if constexpr (LIVE) {
                    const int left = b * 16 + lk + 4 * r < N ? N - (c0 + 2 * li + 32 * g) : 0;   // live entries from here on
                    f64x2 x = {0.0, 0.0};
                    if (left >= 2) x = *reinterpret_cast<const f64x2*>(src);
                    else if (left == 1) x[0] = src[0];
                    v[g][r] = x;
                } else {
                    v[g][r] = *reinterpret_cast<const f64x2*>(src);
                }
            }
    };
    int b = b0 + w;
    if (b < b1) gload(b, cur);
    for (; b < b1; b += 4) {
        if (b + 4 < b1) gload(b + 4, nxt);   // the next block's tile flies under this block's MFMAs
        f64x4 ae[4], ao[4];
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) ae[g][r] = cur[g][r][0], ao[g][r] = cur[g][r][1];
        const double* kg = Kt + b * 16 + li;
        for (int s = 0; s < kp; s += 4) {
            const int k = s + lk;
            double a = k < m ? -kg[(size_t)k * ld] : 0.0;
            if constexpr (LIVE)
                if (b * 16 + li >= N) a = 0.0;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f64x2 tv = *reinterpret_cast<const f64x2*>(dc_smem + k * kUpdCols + 32 * g + 2 * li);
                ae[g] = GemmTraits<double>::mfma(a, tv[0], ae[g]);
                ao[g] = GemmTraits<double>::mfma(a, tv[1], ao[g]);
            }
        }
        double* base = S + (size_t)(b * 16 + lk) * ld + c0 + 2 * li;
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                f64x2 v = {ae[g][r], ao[g][r]};
                double* dst = base + (size_t)(4 * r) * ld + 32 * g;
                if constexpr (LIVE) {
                    const int left = b * 16 + lk + 4 * r < N ? N - (c0 + 2 * li + 32 * g) : 0;
                    if (left >= 2) *reinterpret_cast<f64x2*>(dst) = v;
                    else if (left == 1) dst[0] = v[0];
                } else {
                    *reinterpret_cast<f64x2*>(dst) = v;
                }
            }
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) cur[g][r] = nxt[g][r];
    }
}

size_t panels_lds(int mb) { return sizeof(double) * (size_t)(kTile * kTileS + 2 * kTile * (16 * mb + 2)); }
constexpr size_t kInvertLds = sizeof(double) * (size_t)(kMaxM * kInvS + 4 * kMaxM);
constexpr size_t kUpdateLds = sizeof(double) * (size_t)kMaxM * kUpdCols;

// Launch 6 at rank k: the kernel as it always was when the plan spans the handle (pl.live == 0), the masked one otherwise.
void launch_update(const Dense64CorrectPlan& pl, double* Sigma, const double* Kt, const double* Tp, const int* verdict, int k,
                   hipStream_t s) {
    const size_t lds = sizeof(double) * (size_t)((k + 3) & ~3) * kUpdCols;
    if (pl.live)
        hipLaunchKernelGGL(k_dc_update<true>, dim3(pl.upd_strips, pl.upd_chunks), dim3(256), lds, s, Sigma, Kt, Tp, verdict,
                           pl.N, pl.ld, k, pl.upd_blocks_per_chunk);
    else
        hipLaunchKernelGGL(k_dc_update<false>, dim3(pl.upd_strips, pl.upd_chunks), dim3(256), lds, s, Sigma, Kt, Tp, verdict,
                           pl.N, pl.ld, k, pl.upd_blocks_per_chunk);
}

template <int MB>
void launch_panels(const Dense64CorrectPlan& pl, const double* S, const double* Ht, double* Tpart, double* Upart,
                   hipStream_t s) {
    hipLaunchKernelGGL((k_dc_panels<MB>), dim3(pl.n_strips, pl.n_chunks), dim3(256), panels_lds(MB), s, S, Ht, Tpart,
                       Upart, pl.N, pl.ld, pl.tiles_per_chunk);
}

}  // namespace

hipError_t dense64_correct_prepare() {
    // all of these take more LDS than a kernel may without asking (panels: 51 / 67 / 83 / 99 KiB for m <= 16 / 32 / 48 / 64)
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dc_panels<1>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)panels_lds(1));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dc_panels<2>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)panels_lds(2));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dc_panels<3>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)panels_lds(3));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dc_panels<4>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)panels_lds(4));
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dc_invert), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kInvertLds);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dc_update<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kUpdateLds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dc_update<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kUpdateLds);
}

Dense64CorrectPlan dense64_correct_plan(int N, int ld) {
    Dense64CorrectPlan pl{};
    pl.N = N;
    pl.ld = ld;
    const int strip_cols = kStripTiles * kTile;
    pl.n_strips = (N + strip_cols - 1) / strip_cols;
    const int row_tiles = (N + kTile - 1) / kTile;
    // about two resident workgroups per CU in all (256 CUs), never more chunks than row tiles
    int chunks = 512 / pl.n_strips;
    if (chunks < 1) chunks = 1;
    if (chunks > row_tiles) chunks = row_tiles;
    pl.tiles_per_chunk = (row_tiles + chunks - 1) / chunks;
    pl.n_chunks = (row_tiles + pl.tiles_per_chunk - 1) / pl.tiles_per_chunk;
    pl.n_sparts = (N + 127) / 128;
    pl.upd_strips = (N + kUpdCols - 1) / kUpdCols;
    const int nb = (N + 15) / 16;
    int uch = 512 / pl.upd_strips;
    if (uch < 1) uch = 1;
    if (uch > (nb + 3) / 4) uch = (nb + 3) / 4;
    pl.upd_blocks_per_chunk = (nb + uch - 1) / uch;
    pl.upd_chunks = (nb + pl.upd_blocks_per_chunk - 1) / pl.upd_blocks_per_chunk;
    // workspace, in doubles: T, U^T, K^T panels, the partial panels, the S chunks, S^-1
    const size_t panel = (size_t)kMaxM * ld;
    pl.off_T = 0;
    pl.off_Ut = panel;
    pl.off_Kt = 2 * panel;
    pl.off_Tpart = 3 * panel;
    pl.off_Upart = pl.off_Tpart + (size_t)pl.n_chunks * panel;
    pl.off_Spart = pl.off_Upart + (size_t)pl.n_strips * panel;
    pl.off_Sinv = pl.off_Spart + (size_t)pl.n_sparts * kMaxM * kMaxM;
    pl.ws_doubles = pl.off_Sinv + (size_t)kMaxM * kMaxM;
    return pl;
}

// The plan of the structured calls at live dimension Na <= N: every launch is cut for Na (strips, chunks, the rows of the gain)
// on the handle's ld, and the panels stay where the handle's own plan put them, because the workspace was sized for that.
Dense64CorrectPlan dense64_live_plan(const Dense64CorrectPlan& full, int Na) {
    if (Na >= full.N) return full;
    Dense64CorrectPlan pl = dense64_correct_plan(Na, full.ld);
    pl.live = 1;
    pl.off_T = full.off_T, pl.off_Ut = full.off_Ut, pl.off_Kt = full.off_Kt, pl.off_Tpart = full.off_Tpart;
    pl.off_Upart = full.off_Upart, pl.off_Spart = full.off_Spart, pl.off_Sinv = full.off_Sinv, pl.ws_doubles = full.ws_doubles;
    return pl;
}

void launch_dense64_correct(const Dense64CorrectPlan& pl, double* Sigma, double* state, double* ws, const double* Hd,
                            const double* Ht, const double* R, const double* nu, int m, double* nis, int* verdict,
                            hipStream_t s) {
    double* Tp = ws + pl.off_T;
    double* Ut = ws + pl.off_Ut;
    double* Kt = ws + pl.off_Kt;
    double* Tpart = ws + pl.off_Tpart;
    double* Upart = ws + pl.off_Upart;
    double* Spart = ws + pl.off_Spart;
    double* Sinv = ws + pl.off_Sinv;
    switch ((m + 15) / 16) {
        case 1: launch_panels<1>(pl, Sigma, Ht, Tpart, Upart, s); break;
        case 2: launch_panels<2>(pl, Sigma, Ht, Tpart, Upart, s); break;
        case 3: launch_panels<3>(pl, Sigma, Ht, Tpart, Upart, s); break;
        default: launch_panels<4>(pl, Sigma, Ht, Tpart, Upart, s); break;
    }
    hipLaunchKernelGGL(k_dc_sum, dim3((pl.ld / 2 + 255) / 256, m), dim3(256), 0, s, Tpart, Upart, Tp, Ut, pl.N, pl.ld, m,
                       pl.n_chunks, pl.n_strips);
    hipLaunchKernelGGL(k_dc_spart, dim3(pl.n_sparts), dim3(256), 0, s, Tp, Hd, Spart, pl.ld, m);
    hipLaunchKernelGGL(k_dc_invert, dim3(1), dim3(256), kInvertLds, s, Spart, pl.n_sparts, R, nu, Sinv, nis, verdict, m);
    hipLaunchKernelGGL(k_dc_gain, dim3((pl.N + kGainRows - 1) / kGainRows), dim3(256), 0, s, Ut, Sinv, nu, Kt, state, verdict, pl.N, pl.ld, m);
    launch_update(pl, Sigma, Kt, Tp, verdict, m, s);
}

// Launches 5 and 6 alone, for a caller that has put T, U^T and S^-1 into ws itself (ekf_dense64_sparse.hip).
void launch_dense64_correct_tail(const Dense64CorrectPlan& pl, double* Sigma, double* state, double* ws, const double* nu,
                                 int m, const int* verdict, hipStream_t s) {
    double* Tp = ws + pl.off_T;
    double* Ut = ws + pl.off_Ut;
    double* Kt = ws + pl.off_Kt;
    double* Sinv = ws + pl.off_Sinv;
    hipLaunchKernelGGL(k_dc_gain, dim3((pl.N + kGainRows - 1) / kGainRows), dim3(256), 0, s, Ut, Sinv, nu, Kt, state, verdict, pl.N, pl.ld, m);
    launch_update(pl, Sigma, Kt, Tp, verdict, m, s);
}

// Launch 5 alone, with K^T written to `Kt` instead of the workspace panel (the deferred form of ekf_dense64_sparse.hip: a pending row).
void launch_dense64_gain(const Dense64CorrectPlan& pl, const double* ws, double* Kt, double* state, const double* nu, int m,
                         const int* verdict, hipStream_t s) {
    hipLaunchKernelGGL(k_dc_gain, dim3((pl.N + kGainRows - 1) / kGainRows), dim3(256), 0, s, ws + pl.off_Ut,
                       ws + pl.off_Sinv, nu, Kt, state, verdict, pl.N, pl.ld, m);
}

// Launch 6 alone on the pending panels of p deferred rows: Sigma <- Sigma - sum_q Kp[q]^T Tq[q].  `zero`: a device word
// that holds 0 (the kernel's verdict argument).
void launch_dense64_flush(const Dense64CorrectPlan& pl, double* Sigma, const double* Kp, const double* Tq, int p,
                          const int* zero, hipStream_t s) {
    launch_update(pl, Sigma, Kp, Tq, zero, p, s);
}

}  // namespace ekf
