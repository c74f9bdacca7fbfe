// ekf_dense64_joseph.hip -- the Joseph form of the sparse measurement update of the dense fp64 handle, with per-state gain
// weights (ekf_dense64_correct_sparse_joseph, include/ekfslam.h):
//   K = diag(w) U S^-1      D = U - K S      state += K nu      Sigma <- Sigma - K T - D K^T
// which is (I - K H) Sigma (I - K H)^T + K R K^T written with the panels the short form already has: T = H Sigma, U = Sigma H^T
// and S = T H^T + R come from the gather and the scoring kernel of ekf_dense64_sparse.hip as they stand, S^-1 and the verdict
// from the elimination of ekf_dense64_invert.hpp behind them.  D is the residual of the gain equation: zero up to rounding for
// the optimal gain (w = 1), U itself where w = 0.  A state with w = 0 is a CONSIDER state: its estimate and its own block of
// Sigma stay as they are, its cross-covariances with the active states are updated.
//   1 k_dj_gain     32 rows of K per workgroup as k_dc_gain (ekf_dense64_correct.hip): G = U S^-1 in that kernel's order, K =
//                   w G (+0.0 where w = 0), state += K nu in that kernel's fold where w != 0, D by one fused multiply-add per
//                   l on an accumulator that starts at U.  Writes the LEFT panel [K^T ; D^T] where the short form keeps K^T
//                   and K^T again under T, which makes the RIGHT panel [T ; K^T]: 2 m rows each in the [k][ld] layout.  Also
//                   one byte per state (w != 0) and the activity bytes of the state's 16-row block and 128-column strip.
//   2 k_dj_update   the access pattern of k_dc_update: a workgroup takes a strip of 128 columns, whose right panel sits in LDS,
//                   and a chunk of 16-row blocks dealt to its four waves; a lane owns adjacent column pairs; the next block's
//                   tile flies under this block's v_mfma_f64_16x16x4_f64 chain, whose accumulator is the Sigma tile.  Per
//                   tile the two activity bytes decide (scalar branches): no active row and no active column -- the tile is
//                   neither loaded nor stored; no active row -- the D K^T chain alone; no active column -- the K T chain
//                   alone.  Inside a mixed tile the zeros of K do the rest, except for an entry whose row and column are both
//                   considered: its store is masked, so whatever it holds (a NaN, an Inf, -0.0) keeps its bits.
// The order inside an entry: the accumulator starts at Sigma[i][j], takes the K T terms (k ascending in fours, one MFMA per
// four) and then the D K^T terms.  No atomics on floating-point data; a run repeats bit for bit.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense_gemm.hpp"   // f64x4, f64x2, GemmTraits<double>::mfma

namespace ekf {

namespace {

constexpr int kPanelRows = kDense64MaxM;       // 64: row stride of S^-1 and the rows of a panel
constexpr int kJM = kDense64JosephMaxM;        // 32
constexpr int kCols = kDense64JosephTileCols;  // 128
constexpr int kRows = kDense64JosephTileRows;  // 16
constexpr int kGainRows = 32;                  // rows of K per workgroup of the gain kernel
static_assert(2 * kJM <= kPanelRows && kCols % kGainRows == 0 && kGainRows == 2 * kRows, "the stacked panels and the bytes");

// ---- 1: K, the state, D, the two stacked panels, the activity bytes ----------------------------------------------------------
// Ut [m][ld], Sinv [64][64] (stride 64), Ssum [m][m]: as the gather and the scoring kernel left them.  w: [N] or NULL (all 1).
// Left [64][ld]: rows k < m become K^T, rows m + k become D^T.  Right [64][ld]: rows k < m hold T already, rows m + k become
// K^T.  Entries at i >= N of the workgroup's 32 rows are written as zeros.
__global__ __launch_bounds__(256) void k_dj_gain(const double* __restrict__ Ut, const double* __restrict__ Sinv,
                                                 const double* __restrict__ Ssum, const double* __restrict__ nu,
                                                 const double* __restrict__ w, double* __restrict__ Left,
                                                 double* __restrict__ Right, double* __restrict__ state,
                                                 unsigned char* __restrict__ state_on, unsigned char* __restrict__ block,
                                                 unsigned char* __restrict__ strip, const int* __restrict__ verdict, int N,
                                                 int ld, int m) {
    __shared__ double si[kJM][kJM + 1], ss[kJM][kJM + 1], ul[kJM][kGainRows], kl[kJM][kGainRows], sp[8][kGainRows];
    __shared__ int act[6];   // [2 h], [2 h + 1]: half h of the rows has a w != 0, a w == 0; [4], [5]: the strip
    if (verdict[0] != 0) return;   // (uniform) the decision precedes every write
    const int t = threadIdx.x, i = t & (kGainRows - 1), g = t / kGainRows;   // g: 8 groups, k = g + 8 q
    const int i0 = blockIdx.x * kGainRows;
    if (t < 6) act[t] = 0;
    for (int e = t; e < kJM * kJM; e += 256) {
        const int l = e / kJM, k = e % kJM;
        const bool in = l < m && k < m;
        si[l][k] = in ? Sinv[l * kPanelRows + k] : 0.0;
        ss[l][k] = in ? Ssum[l * m + k] : 0.0;
    }
    for (int e = t; e < m * kGainRows; e += 256)
        ul[e / kGainRows][e % kGainRows] = Ut[(size_t)(e / kGainRows) * ld + i0 + e % kGainRows];
    __syncthreads();
    const bool real = i0 + i < N;
    const double wi = (w && real) ? w[i0 + i] : 1.0;
    const bool on = real && wi != 0.0;
    if (g == 0 && real) atomicOr(&act[2 * (i / kRows) + (on ? 0 : 1)], 1);
    if (i0 % kCols == 0 && t < kCols && i0 + t < N)   // the first workgroup of a strip looks at the strip's weights
        atomicOr(&act[4 + ((w ? w[i0 + t] : 1.0) != 0.0 ? 0 : 1)], 1);
    double acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = 0.0;
    for (int l = 0; l < m; l++) {
        const double u = ul[l][i];
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] += u * si[l][g + 8 * q];
    }
    double part = 0.0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int k = g + 8 * q;
        if (k < m) {
            const double v = on ? wi * acc[q] : 0.0;   // +0.0 for a consider state and for K's padding
            Left[(size_t)k * ld + i0 + i] = v;
            Right[(size_t)(m + k) * ld + i0 + i] = v;
            kl[k][i] = v;
            if (nu) part += v * nu[k];
        }
    }
    sp[g][i] = part;
    __syncthreads();
    if (g == 0) {
        state_on[i0 + i] = on ? 1 : 0;
        if (nu && on) {   // a consider state is not written
            double v = sp[0][i];
#pragma unroll
            for (int q = 1; q < 8; q++) v += sp[q][i];
            state[i0 + i] = state[i0 + i] + v;
        }
    }
    if (t < 2) block[i0 / kRows + t] = (unsigned char)(act[2 * t] | (act[2 * t + 1] << 1));
    if (t == 2 && i0 % kCols == 0) strip[i0 / kCols] = (unsigned char)(act[4] | (act[5] << 1));
    // D[i][k] = U[i][k] - sum_l K[i][l] S[l][k], one fused multiply-add per l
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int k = g + 8 * q;
        if (k < m) {
            double d = ul[k][i];
            for (int l = 0; l < m; l++) d = fma(-kl[l][i], ss[l][k], d);
            Left[(size_t)(m + k) * ld + i0 + i] = real ? d : 0.0;
        }
    }
}

// ---- 2: Sigma <- Sigma - K T - D K^T ------------------------------------------------------------------------------------------
// The lane maps are k_dc_update's: lane (lk, li) of a wave owns rows lk + 4 r of its 16-row block and, in each of the four
// column groups, the ADJACENT columns 32 g + 2 li, + 1 (one 16-byte access), which the group's two MFMAs see as their column
// li; the right panel is read from LDS with the same pairing.  LDS: [2 kp][128], kp = m rounded up to 4 with zero fill: rows
// < kp are T, rows kp .. are K^T at the strip's columns (filled only when the strip has an active column).  Whatever the
// panels hold at indices >= N is not this call's and enters as +0.  LIVE: N is below the handle's capacity, so rows and
// columns >= N of Sigma are the tail that the call neither reads nor writes, masked element by element as in
// k_dc_update<true>; LIVE = false: they are the padding up to ld, which holds zeros and takes part.
template <bool LIVE>
__global__ __launch_bounds__(kDense64JosephThreads) void k_dj_update(
    double* __restrict__ S, const double* __restrict__ Left, const double* __restrict__ Right,
    const unsigned char* __restrict__ state_on, const unsigned char* __restrict__ block,
    const unsigned char* __restrict__ strip, const int* __restrict__ verdict, int N, int ld, int m, int blocks_per_chunk) {
    extern __shared__ __attribute__((aligned(16))) double dj_smem[];   // [2 kp][128]
    if (verdict[0] != 0) return;   // (uniform) the decision precedes every write
    const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int li = lane & 15, lk = lane >> 4;
    const int kp = (m + 3) & ~3;
    const int c0 = blockIdx.x * kCols;
    const int sb = strip[blockIdx.x];
    const bool col_on = (sb & 1) != 0, col_zero = (sb & 2) != 0;   // (uniform)
    const int nb = (N + kRows - 1) / kRows;
    const int b0 = blockIdx.y * blocks_per_chunk;
    const int b1 = min(nb, b0 + blocks_per_chunk);
    // a tile is touched when its row block or its strip has an active state
    auto next_tile = [&](int b) {
        if (!col_on)
            while (b < b1 && !(__builtin_amdgcn_readfirstlane((int)block[b]) & 1)) b += 4;
        return b;
    };
    for (int e = t; e < 2 * kp * (kCols / 2); e += kDense64JosephThreads) {
        const int k = e / (kCols / 2), c2 = (e % (kCols / 2)) * 2;
        const int src = k < kp ? (k < m ? k : -1) : (col_on && k - kp < m ? m + k - kp : -1);   // row of the right panel
        f64x2 v = {0.0, 0.0};
        if (src >= 0) v = *reinterpret_cast<const f64x2*>(Right + (size_t)src * ld + c0 + c2);
        if (c0 + c2 >= N) v[0] = 0.0;
        if (c0 + c2 + 1 >= N) v[1] = 0.0;
        *reinterpret_cast<f64x2*>(dj_smem + k * kCols + c2) = v;
    }
    __syncthreads();
    unsigned cz = 0;   // bit 2 g + e: the lane's column 32 g + 2 li + e belongs to a consider state
    if (col_zero) {
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const int j = c0 + 32 * g + 2 * li + e;
                if (j < N && state_on[j] == 0) cz |= 1u << (2 * g + e);
            }
    }

    f64x2 cur[4][4], nxt[4][4];
    auto gload = [&](int b, f64x2 (&v)[4][4]) {
        const double* base = S + (size_t)(b * kRows + lk) * ld + c0 + 2 * li;
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const double* src = base + (size_t)(4 * r) * ld + 32 * g;
                if constexpr (LIVE) {
                    const int left = b * kRows + lk + 4 * r < N ? N - (c0 + 2 * li + 32 * g) : 0;   // live entries from here on
                    f64x2 x = {0.0, 0.0};
                    if (left >= 2) x = *reinterpret_cast<const f64x2*>(src);
                    else if (left == 1) x[0] = src[0];
                    v[g][r] = x;
                } else {
                    v[g][r] = *reinterpret_cast<const f64x2*>(src);
                }
            }
    };
    int b = next_tile(b0 + w);
    if (b < b1) gload(b, cur);
    while (b < b1) {
        const int bn = next_tile(b + 4);
        if (bn < b1) gload(bn, nxt);   // the next tile flies under this tile's MFMAs
        const int rb = __builtin_amdgcn_readfirstlane((int)block[b]);
        f64x4 ae[4], ao[4];
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) ae[g][r] = cur[g][r][0], ao[g][r] = cur[g][r][1];
        // the stacked rank: rows [0, kp) of the LDS panel are the K T terms (left operand K^T), rows [kp, 2 kp) the D K^T
        // terms (left operand D^T); the tile's two bytes choose the range (uniform)
        const bool row_real = b * kRows + li < N;
        const double* lg = Left + b * kRows + li;
        const int s_end = col_on ? 2 * kp : kp;
        for (int s = (rb & 1) ? 0 : kp; s < s_end; s += 4) {
            const int kk = s + lk, k = kk < kp ? kk : kk - kp;
            const double a = (k < m && row_real) ? -lg[(size_t)(kk < kp ? k : m + k) * ld] : 0.0;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f64x2 tv = *reinterpret_cast<const f64x2*>(dj_smem + kk * kCols + 32 * g + 2 * li);
                ae[g] = GemmTraits<double>::mfma(a, tv[0], ae[g]);
                ao[g] = GemmTraits<double>::mfma(a, tv[1], ao[g]);
            }
        }
        double* base = S + (size_t)(b * kRows + lk) * ld + c0 + 2 * li;
        if (col_zero && (rb & 2)) {   // (uniform) the tile may hold entries whose row and column are both considered
            unsigned rz = 0;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = b * kRows + lk + 4 * r;
                if (row < N && state_on[row] == 0) rz |= 1u << r;
            }
#pragma unroll
            for (int g = 0; g < 4; g++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    double* dst = base + (size_t)(4 * r) * ld + 32 * g;
                    int left = 2;
                    if constexpr (LIVE) left = b * kRows + lk + 4 * r < N ? N - (c0 + 2 * li + 32 * g) : 0;
                    const bool held = (rz >> r) & 1u;
                    const bool s0 = left >= 1 && !(held && ((cz >> (2 * g)) & 1u));
                    const bool s1 = left >= 2 && !(held && ((cz >> (2 * g + 1)) & 1u));
                    if (s0 && s1) *reinterpret_cast<f64x2*>(dst) = f64x2{ae[g][r], ao[g][r]};
                    else if (s0) dst[0] = ae[g][r];
                    else if (s1) dst[1] = ao[g][r];
                }
        } else {
#pragma unroll
            for (int g = 0; g < 4; g++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const f64x2 v = {ae[g][r], ao[g][r]};
                    double* dst = base + (size_t)(4 * r) * ld + 32 * g;
                    if constexpr (LIVE) {
                        const int left = b * kRows + lk + 4 * r < N ? N - (c0 + 2 * li + 32 * g) : 0;
                        if (left >= 2) *reinterpret_cast<f64x2*>(dst) = v;
                        else if (left == 1) dst[0] = v[0];
                    } else {
                        *reinterpret_cast<f64x2*>(dst) = v;
                    }
                }
        }
#pragma unroll
        for (int g = 0; g < 4; g++)
#pragma unroll
            for (int r = 0; r < 4; r++) cur[g][r] = nxt[g][r];
        b = bn;
    }
}

constexpr size_t kUpdateLds = sizeof(double) * (size_t)2 * kJM * kCols;

}  // namespace

hipError_t dense64_joseph_prepare() {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dj_update<false>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kUpdateLds);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dj_update<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kUpdateLds);
}

Dense64JosephWs dense64_joseph_ws(const Dense64CorrectPlan& pl, double* ws) {
    // ld + 1024 doubles and ld (1 + 1 / 16 + 1 / 128) bytes of the first partial panel's 64 ld doubles
    double* base = ws + pl.off_Tpart;
    unsigned char* bytes = reinterpret_cast<unsigned char*>(base + pl.ld + kJM * kJM);
    return {base, base + pl.ld, bytes, bytes + pl.ld, bytes + pl.ld + pl.ld / kRows};
}

void launch_dense64_correct_sparse_joseph(const Dense64CorrectPlan& pl, double* Sigma, double* state, double* ws,
                                          const int* cols, const double* Hc, const double* R, const double* nu,
                                          const double* w, int m, int s, double* nis, int* verdict, hipStream_t st) {
    const Dense64JosephWs j = dense64_joseph_ws(pl, ws);
    double* Left = ws + pl.off_Kt;
    double* Right = ws + pl.off_T;
    launch_dense64_sparse_panels(pl, Sigma, ws, cols, Hc, R, nu, m, s, nis, j.S, verdict, st);
    hipLaunchKernelGGL(k_dj_gain, dim3((pl.N + kGainRows - 1) / kGainRows), dim3(256), 0, st, ws + pl.off_Ut,
                       ws + pl.off_Sinv, j.S, nu, w, Left, Right, state, j.state_on, j.block, j.strip, verdict, pl.N, pl.ld, m);
    const size_t lds = sizeof(double) * (size_t)2 * ((m + 3) & ~3) * kCols;
    if (pl.live)
        hipLaunchKernelGGL(k_dj_update<true>, dim3(pl.upd_strips, pl.upd_chunks), dim3(kDense64JosephThreads), lds, st, Sigma,
                           Left, Right, j.state_on, j.block, j.strip, verdict, pl.N, pl.ld, m, pl.upd_blocks_per_chunk);
    else
        hipLaunchKernelGGL(k_dj_update<false>, dim3(pl.upd_strips, pl.upd_chunks), dim3(kDense64JosephThreads), lds, st, Sigma,
                           Left, Right, j.state_on, j.block, j.strip, verdict, pl.N, pl.ld, m, pl.upd_blocks_per_chunk);
}

}  // namespace ekf
