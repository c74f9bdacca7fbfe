// ekf_dense_gemm.hpp -- device only: the GEMM behind the dense general-F covariance propagation Sigma <- F * Sigma * F^T + Q
// on the gfx950 matrix cores, written once for the fp32 handle (BASELINE.json configs[3]; SURVEY.md section 8(d) "Dense
// config 4"; held to 1e-4) and the fp64 handle (held to the library's 1e-9 contract).  ekf_dense.hip instantiates both and
// holds the launchers; the cut of a product into tiles is in ekf_dense_split.hpp.
//
// This is the reference's expression `sigma = At*sigma*At.t() + Q` (rigid2d/src/ekf_slam.cpp:101-102) executed the way
// Armadillo executes it -- two dense N x N x N products -- for an ARBITRARY dense At.  (The reference's own At = I + A has
// two off-diagonal non-zeros and is served by the O(N) k_predict kernel; the dense path exists for motion models whose
// Jacobian is a genuine dense matrix, and is the only place on this path where MFMA applies: 4 N^3 flop over 3*4*N^2 bytes
// in fp32, AI ~ 3.3 k flop/B at N = 10003.)
//
//   T      = F * Sigma          "NN": B operand row-major [K][N]
//   Sigma' = T * F^T + Q        "NT": B operand supplied as F[N][K] (k contiguous)
//
// One tile body, gemm_tile: 4 waves as 2 x 2, each owning WTM x WTN accumulators of one MFMA.  Operands go global ->
// registers -> LDS (the next K tile's global loads fly under the MFMAs); LDS images are [k][i] with strides that are odd in
// units of the store width, so that both the transposing stores (of A and of a k-contiguous B) and the fragment reads are
// bank-conflict-free.  Matrices are ld x ld with ld a multiple of 128 and zero padding, so no tile is ragged.
//
// fp32, v_mfma_f32_32x32x2_f32 (exact f32 FMA chains, 64 FLOP/clk/SIMD = the f32 peak): 256 x 128 block tile, BK = 32, a
// wave owns 128 x 64 = 4 x 2 accumulators (128 accumulator registers per lane), one LDS buffer, two workgroups per CU.  Per
// k-step a wave reads WTM + WTN fragment values from LDS for WTM x WTN MFMAs: 4 reads for 4 MFMAs at 2 x 2 (a 128 x 128
// tile), 6 for 8 at 4 x 2 -- and a K tile's staging stores and barriers are shared by twice the matrix work.
// Measured, tools/dense_bench.py at N = 10003: rounds 1-3 ran 128 x 128 tiles, three workgroups per CU, with the tail on a
// second stream: 32.6 ms per propagation (0.76-0.80 of the f32 matrix peak in the steady state of the main kernel itself:
// 4 LDS fragment reads per 4 MFMAs, 32 staging stores and two barriers per 64 MFMAs of a wave).  256 x 128 tiles: 30.7 ms;
// the tail on a lowest-priority second stream: 30.3 ms (its quarter tiles slow the main kernel of the NN product by more
// than their own 0.6 ms when they share the chip with it); the tail behind the main kernel: 30.15 ms = 132.8 TFLOP/s.
//
// fp64, v_mfma_f64_16x16x4_f64 (tools/micro/dense64_tile_ab.hip times it against a register-blocked v_fma_f64 tile of the
// same size; profiles/r05/dense64_tile_ab.txt).  One MFMA is 2048 flop and occupies the DP pipe for tens of cycles, so one
// fragment value per operand per MFMA is far below what LDS delivers: the tile is sized by registers, not by LDS traffic.
// 128 x 128 block tile, BK = 16, a wave owns 64 x 64 = 4 x 4 accumulators (64 doubles = 128 accumulator registers per
// lane), double-buffered LDS (one barrier per K tile), two workgroups per CU.  Measured at N = 10003: 61.4 ms per
// propagation = 65.2 TF = 0.85 of the 77.2 TF the MFMA sustains.
#pragma once
#include <hip/hip_runtime.h>

#include "ekf_dense_split.hpp"

namespace ekf {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// Everything the tile needs to know about an element type: the one MFMA it runs on and that instruction's lane maps.
//   Vec / VW  the 16-byte vector of global loads and of the row-major-B LDS stores, and its length
//   Acc       one accumulator: FR x FR results over 64 lanes
//   FR        edge of the MFMA.  A operand: lane l holds A[i = l & (FR - 1)][k = l / FR]; B: B[k = l / FR][j = l & (FR - 1)]
//   KM        k values per MFMA (64 / FR)
//   SB_PAD    a row-major B is copied with 16-byte stores: pads its LDS row to an odd stride in 16-byte units where needed
//   NBUF      LDS buffers of the main kernel
//   c_row     C/D map: row of register r in a lane of k-group lk (the column is l & (FR - 1))
template <class E> struct GemmTraits;
template <> struct GemmTraits<float> {
    typedef f32x4 Vec;
    typedef f32x16 Acc;
    static constexpr int VW = 4, FR = 32, KM = 2, SB_PAD = 0, NBUF = 1;
    static __device__ __forceinline__ Acc mfma(float a, float b, Acc c) {
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ int c_row(int r, int lk) { return (r & 3) + 8 * (r >> 2) + 4 * lk; }
};
template <> struct GemmTraits<double> {
    typedef f64x2 Vec;
    typedef f64x4 Acc;
    static constexpr int VW = 2, FR = 16, KM = 4, SB_PAD = 2, NBUF = 2;
    static __device__ __forceinline__ Acc mfma(double a, double b, Acc c) {
        return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    }
    // (NOT the map of the f32 16x16x4 instruction)
    static __device__ __forceinline__ int c_row(int r, int lk) { return lk + 4 * r; }
};

// The LDS image of one (2 FR WTM) x (2 FR WTN) tile.  NBUF = 2: double-buffered, one barrier per K tile; NBUF = 1: one
// buffer, two barriers per K tile, half the LDS (more workgroups per CU).
template <class E, bool BT, int NBUF_, int WTM_, int WTN_>
struct GemmTile {
    using TR = GemmTraits<E>;
    static constexpr int NBUF = NBUF_, WTM = WTM_, WTN = WTN_, VW = TR::VW, FR = TR::FR;
    static constexpr int BK = 8 * VW;            // 8 lanes x 16 B cover one row segment of a K tile
    static constexpr int TM = 2 * FR * WTM, TN = 2 * FR * WTN;
    static constexpr int SA = TM + 1;            // odd stride: conflict-free transposing stores and fragment reads
    static constexpr int SB = BT ? TN + 1 : TN + TR::SB_PAD;   // a k-contiguous B is transposed like A; a row-major one is copied
    static constexpr int A_ELEMS = (BK * SA + VW - 1) / VW * VW;   // keeps the B image ...
    static constexpr int B_ELEMS = BK * SB;
    static constexpr int BUF_ELEMS = (A_ELEMS + B_ELEMS + VW - 1) / VW * VW;   // ... and the second buffer 16-B aligned
    static constexpr int PA = TM / 32;           // A staging passes: 32 rows x BK k per pass
    static constexpr int PBT = TN / 32;          // transposed-B staging passes
    static constexpr int RB = 256 * VW / TN;     // row-major B: k rows per pass (256 lanes x 16 B)
    static constexpr int PB = BK / RB;
    static constexpr size_t kLdsBytes = (size_t)NBUF * BUF_ELEMS * sizeof(E);
    static_assert(PA >= 1 && PBT >= 1 && PB >= 1, "tile too small for 256 threads");
};

// the two shapes per element type: the main tile of kDenseMainRows x 128 and the tail's 64 x 64 quarter
template <class E> constexpr int gemm_wt(int edge) { return edge / (2 * GemmTraits<E>::FR); }   // accumulators of a wave along an edge
template <class E, bool BT>
using GemmMainTile = GemmTile<E, BT, GemmTraits<E>::NBUF, gemm_wt<E>(kDenseMainRows<E>), gemm_wt<E>(kDenseTile)>;
template <class E, bool BT>
using GemmTailTile = GemmTile<E, BT, 1, gemm_wt<E>(kDenseQuarter), gemm_wt<E>(kDenseQuarter)>;
// the four shapes in use and their LDS layouts, to the byte (the main kernels: 49.4 KB and 64.8 KiB)
template <class T> constexpr bool gemm_is(int tm, int tn, int nbuf, int wtm, int wtn, size_t lds) {
    return T::TM == tm && T::TN == tn && T::NBUF == nbuf && T::WTM == wtm && T::WTN == wtn && T::kLdsBytes == lds;
}
static_assert(gemm_is<GemmMainTile<float, true>>(256, 128, 1, 4, 2, 49408) && gemm_is<GemmMainTile<float, false>>(256, 128, 1, 4, 2, 49280));
static_assert(gemm_is<GemmTailTile<float, true>>(64, 64, 1, 1, 1, 16640) && gemm_is<GemmTailTile<float, false>>(64, 64, 1, 1, 1, 16512));
static_assert(gemm_is<GemmMainTile<double, true>>(128, 128, 2, 4, 4, 66048) && gemm_is<GemmMainTile<double, false>>(128, 128, 2, 4, 4, 66304));
static_assert(gemm_is<GemmTailTile<double, true>>(64, 64, 1, 2, 2, 16640) && gemm_is<GemmTailTile<double, false>>(64, 64, 1, 2, 2, 16768));

// What a caller may hang on the tile's loads and stores.  The default hangs nothing, and every `if constexpr` below then
// leaves the code as it is written for the propagation.  A mask with kOn (ekf_dense64_region.hip) provides
//   Vec a(const E* p, int row, int k)    the A operand at rows / columns (row, k .. k + VW) of A, p pointing at it
//   Vec b(const E* p, int k, int col)    the row-major B operand at (k, col .. col + VW)
//   bool c(int row, int col)             whether C (and Qadd) at (row, col) is read and written at all
// and answers with zeros instead of loading what does not belong to the product: 0 x NaN is a NaN, so an entry that is to
// stay out must not reach the MFMA.
struct GemmNoMask { static constexpr bool kOn = false; };

// One output tile of (2 FR WTM) x (2 FR WTN) at row0 / col0 of C; smem: GemmTile::kLdsBytes, 16-byte aligned.
template <class E, bool BT, int NBUF, int WTM, int WTN, class Mask = GemmNoMask>
__device__ __forceinline__ void gemm_tile(const E* __restrict__ A, const E* __restrict__ B, E* __restrict__ C,
                                          const E* __restrict__ Qadd, int ld, int row0, int col0, E* smem, int kdim,
                                          Mask mask = Mask()) {
    static_assert(!Mask::kOn || !BT, "a mask is defined for a row-major B");
    using Tile = GemmTile<E, BT, NBUF, WTM, WTN>;
    using TR = GemmTraits<E>;
    using Vec = typename TR::Vec;
    constexpr int VW = Tile::VW, FR = Tile::FR, BK = Tile::BK, TN = Tile::TN, SA = Tile::SA, SB = Tile::SB, PA = Tile::PA,
                  PBT = Tile::PBT, RB = Tile::RB, PB = Tile::PB, A_ELEMS = Tile::A_ELEMS, BUF_ELEMS = Tile::BUF_ELEMS;
    constexpr int NACC = FR * FR / 64;   // registers of one accumulator

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & (FR - 1), lk = lane / FR;
    const E* Ag = A + (size_t)row0 * ld;
    const E* Bg = BT ? B + (size_t)col0 * ld : B + col0;

    Vec ra[PA], rb[BT ? PBT : PB];
    auto gload = [&](int k0) {
#pragma unroll
        for (int p = 0; p < PA; p++) {  // 8 lanes cover one 128-B row segment
            const int row = p * 32 + (t >> 3), kv = (t & 7) * VW;
            if constexpr (Mask::kOn) ra[p] = mask.a(Ag + (size_t)row * ld + k0 + kv, row0 + row, k0 + kv);
            else ra[p] = *reinterpret_cast<const Vec*>(Ag + (size_t)row * ld + k0 + kv);
        }
        if constexpr (BT) {
#pragma unroll
            for (int p = 0; p < PBT; p++) {
                const int row = p * 32 + (t >> 3), kv = (t & 7) * VW;
                rb[p] = *reinterpret_cast<const Vec*>(Bg + (size_t)row * ld + k0 + kv);
            }
        } else {
#pragma unroll
            for (int p = 0; p < PB; p++) {  // TN / VW lanes cover one row segment of the tile
                const int k = p * RB + t / (TN / VW), jv = (t % (TN / VW)) * VW;
                if constexpr (Mask::kOn) rb[p] = mask.b(Bg + (size_t)(k0 + k) * ld + jv, k0 + k, col0 + jv);
                else rb[p] = *reinterpret_cast<const Vec*>(Bg + (size_t)(k0 + k) * ld + jv);
            }
        }
    };
    auto lstore = [&](int buf) {
        E* as = smem + buf * BUF_ELEMS;
        E* bs = as + A_ELEMS;
#pragma unroll
        for (int p = 0; p < PA; p++) {
            const int row = p * 32 + (t >> 3), kv = (t & 7) * VW;
#pragma unroll
            for (int j = 0; j < VW; j++) as[(kv + j) * SA + row] = ra[p][j];
        }
        if constexpr (BT) {
#pragma unroll
            for (int p = 0; p < PBT; p++) {
                const int row = p * 32 + (t >> 3), kv = (t & 7) * VW;
#pragma unroll
                for (int j = 0; j < VW; j++) bs[(kv + j) * SB + row] = rb[p][j];
            }
        } else {
#pragma unroll
            for (int p = 0; p < PB; p++) {
                const int k = p * RB + t / (TN / VW), jv = (t % (TN / VW)) * VW;
                *reinterpret_cast<Vec*>(bs + k * SB + jv) = rb[p];
            }
        }
    };

    typename TR::Acc acc[WTM][WTN];
#pragma unroll
    for (int i = 0; i < WTM; i++)
#pragma unroll
        for (int j = 0; j < WTN; j++)
#pragma unroll
            for (int r = 0; r < NACC; r++) acc[i][j][r] = E(0);

    // (the K range behind N is zero padding in both operands: 316 -> 313 K tiles of 32 at N = 10003)
    const int nk = (kdim + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int cur = NBUF == 2 ? (kt & 1) : 0;
        if (kt + 1 < nk) gload((kt + 1) * BK);  // next tile's global loads fly under this tile's MFMAs
        const E* as = smem + cur * BUF_ELEMS + wm * FR * WTM + li;
        const E* bs = smem + cur * BUF_ELEMS + A_ELEMS + wn * FR * WTN + li;
        // fragments of the next k-step are read from LDS before the MFMAs of this k-step are issued, so the
        // ds_read latency hides under the matrix work instead of stalling in front of it
        E a[WTM], b[WTN];
#pragma unroll
        for (int i = 0; i < WTM; i++) a[i] = as[lk * SA + FR * i];
#pragma unroll
        for (int j = 0; j < WTN; j++) b[j] = bs[lk * SB + FR * j];
#pragma unroll
        for (int kk = 0; kk < BK; kk += TR::KM) {
            E an[WTM], bn[WTN];
#pragma unroll
            for (int i = 0; i < WTM; i++) an[i] = E(0);
#pragma unroll
            for (int j = 0; j < WTN; j++) bn[j] = E(0);
            if (kk + TR::KM < BK) {
#pragma unroll
                for (int i = 0; i < WTM; i++) an[i] = as[(kk + TR::KM + lk) * SA + FR * i];
#pragma unroll
                for (int j = 0; j < WTN; j++) bn[j] = bs[(kk + TR::KM + lk) * SB + FR * j];
            }
            __builtin_amdgcn_sched_barrier(0);  // keep hipcc from sinking the reads back below the MFMAs
#pragma unroll
            for (int i = 0; i < WTM; i++)
#pragma unroll
                for (int j = 0; j < WTN; j++) acc[i][j] = TR::mfma(a[i], b[j], acc[i][j]);
#pragma unroll
            for (int i = 0; i < WTM; i++) a[i] = an[i];
#pragma unroll
            for (int j = 0; j < WTN; j++) b[j] = bn[j];
        }
        if (kt + 1 < nk) {
            if constexpr (NBUF == 2) {
                lstore(cur ^ 1);  // the other buffer was last read one barrier ago
                __syncthreads();
            } else {
                __syncthreads();  // every wave is done reading the only buffer
                lstore(0);
                __syncthreads();
            }
        }
    }

    E* Cg = C + (size_t)(row0 + wm * FR * WTM) * ld + col0 + wn * FR * WTN;
    const E* Qg = Qadd ? Qadd + (size_t)(row0 + wm * FR * WTM) * ld + col0 + wn * FR * WTN : nullptr;
#pragma unroll
    for (int i = 0; i < WTM; i++)
#pragma unroll
        for (int j = 0; j < WTN; j++)
#pragma unroll
            for (int r = 0; r < NACC; r++) {
                const int row = i * FR + TR::c_row(r, lk);
                const int col = j * FR + li;
                if constexpr (Mask::kOn)
                    if (!mask.c(row0 + wm * FR * WTM + row, col0 + wn * FR * WTN + col)) continue;
                E v = acc[i][j][r];
                if (Qg) v += Qg[(size_t)row * ld + col];
                Cg[(size_t)row * ld + col] = v;
            }
}

// The main kernel: ids [0, sp.n_big) of the grouped tile list, two workgroups per CU.
// fp32 at N = 10003 (ld = 10112): 39 x 79 = 3081 tiles of 256 x 128 over 512 resident workgroup slots = 6 whole rounds
// (3072 tiles); the other 9 main tiles (18 tiles of 128 x 128) and the bottom strip (79 tiles of 128 x 128: ld is
// 39.5 x 256) are cut into 64 x 64 quarters on the tail kernel, which follows on the same stream (0.55-0.62 ms; quarters
// that hold padding rows only are skipped) -- behind the main kernel and not beside it: see the measurements at the top.
template <class E, bool BT>
__global__ __launch_bounds__(256, 2) void k_gemm_big(const E* __restrict__ A, const E* __restrict__ B, E* __restrict__ C,
                                                     const E* __restrict__ Qadd, DenseSplit sp) {
    using Tile = GemmMainTile<E, BT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char gemm_smem[];
    int tm, tn;
    big_tile_of(xcd_remap(blockIdx.x, sp.n_big), sp.tiles_m, sp.tiles_n, tm, tn);
    gemm_tile<E, BT, Tile::NBUF, Tile::WTM, Tile::WTN>(
        A, B, C, Qadd, sp.ld, tm * Tile::TM, tn * Tile::TN, reinterpret_cast<E*>(gemm_smem), sp.n_rows);
}

// The tail kernel: small tile s >> 2 of the split, quarter s & 3.
template <class E, bool BT>
__global__ __launch_bounds__(256, 4) void k_gemm_tail(const E* __restrict__ A, const E* __restrict__ B, E* __restrict__ C,
                                                      const E* __restrict__ Qadd, DenseSplit sp) {
    using Tile = GemmTailTile<E, BT>;
    extern __shared__ __attribute__((aligned(16))) unsigned char gemm_smem[];
    const int s = blockIdx.x;
    int row0, col0;
    small_tile_origin<E>(sp, s >> 2, row0, col0);
    row0 += ((s >> 1) & 1) * Tile::TM;
    if (row0 >= sp.n_rows) return;   // (uniform) padding rows only: at N = 10003 half of the bottom strip's quarters
    gemm_tile<E, BT, Tile::NBUF, Tile::WTM, Tile::WTN>(
        A, B, C, Qadd, sp.ld, row0, col0 + (s & 1) * Tile::TN, reinterpret_cast<E*>(gemm_smem), sp.n_rows);
}

}  // namespace ekf
