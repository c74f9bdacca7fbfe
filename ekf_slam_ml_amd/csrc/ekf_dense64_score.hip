// ekf_dense64_score.hip -- batched Mahalanobis scoring of J candidate measurements against the dense fp64 covariance,
// read-only: the reference's calculate_maha_dis (rigid2d/src/ekf_slam.cpp:217-276)
//   psi = Hj*sigma*Hj.t() + R;   d = nu^T psi^-1 nu
// for J arbitrary m x N Jacobians in one pass over Sigma.  Three launches on one stream, no floating-point atomics:
//   1 k_ds_panels   candidates are packed whole into row groups of up to 64 rows (floor(64 / m) candidates; a candidate's
//                   rows never straddle two groups).  A workgroup owns (group, strip of up to four 64-column tiles, chunk
//                   of 64-row tiles of Sigma) -- the cut of k_dc_panels, a function of (N, ld) alone.  It walks the chunk's
//                   rows of Sigma in that strip once, each 64 x 64 tile global -> registers -> LDS, and builds the group's
//                   slice of T = H Sigma in v_mfma_f64_16x16x4_f64 accumulators (T[:, J] += H[:, I] Sigma[I, J]).  The
//                   slice then goes accumulators -> LDS (never to memory) and is contracted with the same strip of H^T on
//                   the matrix cores into a 64 x 64 product whose diagonal m x m blocks are the candidates' partial S.
//   2 k_ds_sum      the n_chunks * n_strips partial blocks of every candidate summed in index order, a thread per element
//   3 k_ds_invert   per candidate: S = that sum + R, the elimination of ekf_dense64_invert.hpp (the one k_dc_invert
//                   uses), flag, nis.  m <= 16: a wave per candidate, four to a workgroup; above: a workgroup each.
// An MFMA row depends on no other row, the k order is fixed by (N, ld) and a candidate's partial blocks are summed in
// the same order wherever it sits, so its outputs are the same bits alone, at any position of any batch with the same
// m, and from run to run.  Rows of a group that hold no candidate are loaded as zeros; what they (or a candidate full of
// NaN) produce lies outside every other candidate's diagonal block and is not stored.
// Group of 64 rows and not 128: see DESIGN.md 4.8.3 (16 flop per byte of Sigma is already above the machine's
// 78.6 TF / 8 TB/s = 9.8, the groups of one super-tile are adjacent in the grid and share it through L2 / MALL, and 128
// rows would double the accumulators to 256 registers and halve the occupancy that hides the tile loads).
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"
#include "ekf_dense_gemm.hpp"   // f64x4, f64x2, GemmTraits<double>::mfma
#include "ekf_dense64_invert.hpp"

namespace ekf {

namespace {

constexpr int kMaxM = kDense64MaxM;
constexpr int kGroup = kDense64ScoreGroup;   // rows of H per group
constexpr int kTile = 64;
constexpr int kTileS = kTile + 2;            // as k_dc_panels
constexpr int kStripTiles = 4;

// Hs: the stacked Jacobians, [n_groups * 64][ld] row-major, row g * 64 + q * m + r = row r of candidate g * cpg + q;
// columns N .. ld are zero.  Spart: [n_chunks * n_strips][J][m * m].
template <int MB>
__global__ __launch_bounds__(256) void k_ds_panels(const double* __restrict__ S, const double* __restrict__ Hs,
                                                   double* __restrict__ Spart, int N, int ld, int tiles_per_chunk,
                                                   int n_strips, int m, int J, int cpg) {
    constexpr int HS = 16 * MB + 2;   // LDS row stride of the H tile
    extern __shared__ __attribute__((aligned(16))) double ds_smem[];
    double* tile = ds_smem;                 // [64][kTileS]: a tile of Sigma, later a tile of T
    double* ht = tile + kTile * kTileS;     // [64 k][16 MB]: H[group rows, 64 columns]^T

    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int group = blockIdx.x, strip = blockIdx.y, chunk = blockIdx.z;
    const int col_base = strip * kStripTiles * kTile;
    const int n_row_tiles = (N + kTile - 1) / kTile;
    const int rt0 = chunk * tiles_per_chunk;
    const int rt1 = min(n_row_tiles, rt0 + tiles_per_chunk);
    int nct = (N - col_base + kTile - 1) / kTile;   // column tiles of this strip that hold real columns
    if (nct > kStripTiles) nct = kStripTiles;
    const int rows_g = min(cpg, J - group * cpg) * m;   // rows of this group that hold a candidate
    if (rt0 >= rt1 || nct <= 0 || rows_g <= 0) return;  // (uniform; the host launches no such workgroup)
    const double* Hg = Hs + (size_t)group * kGroup * ld;

    f64x2 pre[8];
    auto gload = [&](int rt, int ct) {
        const double* g = S + (size_t)(rt * kTile) * ld + col_base + ct * kTile;
#pragma unroll
        for (int p = 0; p < 8; p++)
            pre[p] = *reinterpret_cast<const f64x2*>(g + (size_t)((t >> 5) + 8 * p) * ld + (t & 31) * 2);
    };
    auto hload = [&](int first) {   // ht[k][i] = H[group row i][first + k], zero for rows without a candidate
        for (int e = t; e < 16 * MB * 32; e += 256) {
            const int row = e >> 5, c2 = (e & 31) * 2;
            f64x2 v = {0.0, 0.0};
            if (row < rows_g) v = *reinterpret_cast<const f64x2*>(Hg + (size_t)row * ld + first + c2);
            ht[c2 * HS + row] = v[0];
            ht[(c2 + 1) * HS + row] = v[1];
        }
    };

    f64x4 accT[kStripTiles][MB];
#pragma unroll
    for (int c = 0; c < kStripTiles; c++)
#pragma unroll
        for (int b = 0; b < MB; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) accT[c][b][r] = 0.0;

    gload(rt0, 0);
    for (int rt = rt0; rt < rt1; rt++) {
#pragma unroll
        for (int ct = 0; ct < kStripTiles; ct++) {
            if (ct < nct) {   // (uniform)
                __syncthreads();   // every wave is done reading the previous tile
#pragma unroll
                for (int p = 0; p < 8; p++)
                    *reinterpret_cast<f64x2*>(tile + ((t >> 5) + 8 * p) * kTileS + (t & 31) * 2) = pre[p];
                if (ct == 0) hload(rt * kTile);
                __syncthreads();
                // the next tile's global loads fly under this tile's MFMAs
                if (ct + 1 < nct) gload(rt, ct + 1);
                else if (rt + 1 < rt1) gload(rt + 1, 0);
                // T[i][j] += H[i][k] Sigma[k][j]: wave w owns the 16 columns j = 16 w + (0..15) of the tile
#pragma unroll 4
                for (int s = 0; s < kTile / 4; s++) {
                    const double b = tile[(4 * s + lk) * kTileS + 16 * w + li];
#pragma unroll
                    for (int kb = 0; kb < MB; kb++)
                        accT[ct][kb] = GemmTraits<double>::mfma(ht[(4 * s + lk) * HS + 16 * kb + li], b, accT[ct][kb]);
                }
            }
        }
    }

    // ---- the slice of T meets the same strip of H^T: P[i][l] = sum over the strip's columns j (ascending) T[i][j] H[l][j]
    f64x4 accS[MB];
#pragma unroll
    for (int b = 0; b < MB; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) accS[b][r] = 0.0;
#pragma unroll
    for (int ct = 0; ct < kStripTiles; ct++) {
        if (ct < nct) {   // (uniform)
            __syncthreads();
#pragma unroll
            for (int kb = 0; kb < MB; kb++)
#pragma unroll
                for (int r = 0; r < 4; r++) tile[(16 * kb + lk + 4 * r) * kTileS + 16 * w + li] = accT[ct][kb][r];
            hload(col_base + ct * kTile);   // ht[j][l]
            __syncthreads();
            if (w < MB) {   // (uniform per wave) wave w owns the 16 columns l = 16 w + (0..15) of P
#pragma unroll 4
                for (int s = 0; s < kTile / 4; s++) {
                    const double b = ht[(4 * s + lk) * HS + 16 * w + li];
#pragma unroll
                    for (int kb = 0; kb < MB; kb++)
                        accS[kb] = GemmTraits<double>::mfma(tile[(16 * kb + li) * kTileS + 4 * s + lk], b, accS[kb]);
                }
            }
        }
    }
    if (w < MB) {
        const int l = 16 * w + li;
        const size_t part = (size_t)chunk * n_strips + strip;
        double* out = Spart + (part * J + (size_t)group * cpg) * (size_t)(m * m);
        if (l < rows_g) {
            const int ql = l / m, rl = l - ql * m;
#pragma unroll
            for (int kb = 0; kb < MB; kb++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = 16 * kb + lk + 4 * r;
                    if (i < rows_g && i / m == ql) out[(size_t)ql * (m * m) + (i - ql * m) * m + rl] = accS[kb][r];
                }
        }
    }
}

// ---- 3: per candidate S = sum + R, flag, nis -----------------------------------------------------------------------------------
// NT threads per candidate, 256 / NT candidates per workgroup.  LDS per candidate: [m][2 m + 1] | 2 m | m | m | 1 doubles,
// then the control words of all candidates of the workgroup.
__host__ __device__ constexpr int invert_doubles(int mcap) { return mcap * (2 * mcap + 1) + 4 * mcap + 1; }

// ---- 2: Ssum[cand][e] = the n_parts partial blocks summed in index order; one thread per element, eight loads in flight
__global__ __launch_bounds__(256) void k_ds_sum(const double* __restrict__ Spart, double* __restrict__ Ssum, int n_parts,
                                                size_t total) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const double* p = Spart + e;
    double v = 0.0;
    int c = 0;
    for (; c + 8 <= n_parts; c += 8) {
        double x[8];
#pragma unroll
        for (int q = 0; q < 8; q++) x[q] = p[(size_t)(c + q) * total];
#pragma unroll
        for (int q = 0; q < 8; q++) v += x[q];
    }
    for (; c < n_parts; c++) v += p[(size_t)c * total];
    Ssum[e] = v;
}

template <int NT, int MCAP>
__global__ __launch_bounds__(256) void k_ds_invert(const double* __restrict__ R, int r_shared,
                                                   const double* __restrict__ nu, double* __restrict__ nis,
                                                   double* __restrict__ S_io, int* __restrict__ flag, int m, int J) {
    extern __shared__ __attribute__((aligned(16))) double ds_smem[];
    constexpr int PER = 256 / NT;
    const int sub = threadIdx.x / NT, t = threadIdx.x % NT;
    const int cand = blockIdx.x * PER + sub;
    if (cand >= J) return;   // (uniform over the candidate's thread group; NT = 64 takes no workgroup barrier)
    const int stride = 2 * m + 1;
    double* M = ds_smem + sub * invert_doubles(MCAP);
    double* tail = M + MCAP * (2 * MCAP + 1);
    int* ctl = reinterpret_cast<int*>(ds_smem + PER * invert_doubles(MCAP)) + 2 * sub;
    const GjScratch sc{tail, tail + 2 * MCAP, tail + 3 * MCAP, tail + 4 * MCAP, ctl};
    const int mm = m * m;
    const double* Rc = R + (r_shared ? 0 : (size_t)cand * mm);
    int bad = 0;
    for (int e = t; e < mm; e += NT) {
        const int k = e / m, l = e % m;
        const double v = S_io[(size_t)cand * mm + e] + Rc[e];
        if (!isfinite(v)) bad = 1;
        S_io[(size_t)cand * mm + e] = v;
        M[k * stride + l] = v;
        M[k * stride + m + l] = k == l ? 1.0 : 0.0;
    }
    const int verdict = gj_invert<NT>(M, stride, sc, m, t, bad);   // (uniform over the group)
    double v = __builtin_nan("");
    if (nis && !verdict) v = gj_quadratic<NT>(M, stride, sc, m, t, nu + (size_t)cand * m);
    if (t == 0) {
        if (nis) nis[cand] = v;
        flag[cand] = verdict;
    }
}

constexpr int kWaveM = 16;   // up to here a wave per candidate
size_t panels_lds(int mb) { return sizeof(double) * (size_t)(kTile * kTileS + kTile * (16 * mb + 2)); }
constexpr size_t invert_lds(int nt, int mcap) {
    return sizeof(double) * (size_t)((256 / nt) * invert_doubles(mcap) + (256 / nt));
}

template <int MB>
void launch_panels(const Dense64CorrectPlan& pl, const double* S, const double* Hs, double* Spart, int m, int J, int cpg,
                   int n_groups, hipStream_t s) {
    hipLaunchKernelGGL((k_ds_panels<MB>), dim3(n_groups, pl.n_strips, pl.n_chunks), dim3(256), panels_lds(MB), s, S, Hs,
                       Spart, pl.N, pl.ld, pl.tiles_per_chunk, pl.n_strips, m, J, cpg);
}

template <int MB>
hipError_t raise_panels() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ds_panels<MB>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)panels_lds(MB));
}

}  // namespace

hipError_t dense64_score_prepare() {
    // panels: 41 / 49 / 57 / 65 KiB for up to 16 / 32 / 48 / 64 rows in a group; the workgroup inversion 67 KiB
    hipError_t e = raise_panels<1>();
    if (e != hipSuccess) return e;
    e = raise_panels<2>();
    if (e != hipSuccess) return e;
    e = raise_panels<3>();
    if (e != hipSuccess) return e;
    e = raise_panels<4>();
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ds_invert<64, kWaveM>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)invert_lds(64, kWaveM));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_ds_invert<256, kMaxM>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)invert_lds(256, kMaxM));
}

Dense64ScorePlan dense64_score_plan(int N, int ld, int J, int m) {
    Dense64ScorePlan sp{};
    sp.panels = dense64_correct_plan(N, ld);   // strips and chunks: a function of (N, ld) alone
    sp.cpg = kGroup / m;
    sp.n_groups = (J + sp.cpg - 1) / sp.cpg;
    sp.n_parts = sp.panels.n_chunks * sp.panels.n_strips;
    sp.h_doubles = (size_t)sp.n_groups * kGroup * ld;
    sp.spart_doubles = (size_t)sp.n_parts * J * m * m;
    return sp;
}

void launch_dense64_score(const Dense64ScorePlan& sp, const double* Sigma, const double* Hs, double* Spart,
                          const double* R, int r_shared, const double* nu, int J, int m, double* nis, double* S_io,
                          int* flag, hipStream_t s) {
    const int rows = (J < sp.cpg ? J : sp.cpg) * m;   // of a full group (of the only group, when it is not full)
    switch ((rows + 15) / 16) {
        case 1: launch_panels<1>(sp.panels, Sigma, Hs, Spart, m, J, sp.cpg, sp.n_groups, s); break;
        case 2: launch_panels<2>(sp.panels, Sigma, Hs, Spart, m, J, sp.cpg, sp.n_groups, s); break;
        case 3: launch_panels<3>(sp.panels, Sigma, Hs, Spart, m, J, sp.cpg, sp.n_groups, s); break;
        default: launch_panels<4>(sp.panels, Sigma, Hs, Spart, m, J, sp.cpg, sp.n_groups, s); break;
    }
    const size_t total = (size_t)J * m * m;
    hipLaunchKernelGGL(k_ds_sum, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, Spart, S_io, sp.n_parts, total);
    if (m <= kWaveM)
        hipLaunchKernelGGL((k_ds_invert<64, kWaveM>), dim3((J + 3) / 4), dim3(256), invert_lds(64, kWaveM), s, R, r_shared,
                           nu, nis, S_io, flag, m, J);
    else
        hipLaunchKernelGGL((k_ds_invert<256, kMaxM>), dim3(J), dim3(256), invert_lds(256, kMaxM), s, R, r_shared, nu, nis,
                           S_io, flag, m, J);
}

}  // namespace ekf
