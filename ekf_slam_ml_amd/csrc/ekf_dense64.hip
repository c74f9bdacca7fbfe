// ekf_dense64.hip -- dense general-F covariance propagation Sigma <- F * Sigma * F^T + Q in fp64 on the gfx950 matrix
// cores: the fp64 twin of ekf_dense.hip, held to the library's 1e-9 contract instead of fp32's 1e-4.
//
// Same expression, same two products (the reference's `sigma = At*sigma*At.t() + Q`, rigid2d/src/ekf_slam.cpp:101-102):
//   T      = F * Sigma          "NN": B operand row-major [K][N]
//   Sigma' = T * F^T + Q        "NT": B operand supplied as F[N][K] (k contiguous)
// All values fp64 in HBM, all accumulation fp64.
//
// Instruction: v_mfma_f64_16x16x4_f64 (tools/micro/dense64_tile_ab.hip times it against a register-blocked v_fma_f64 tile
// of the same size; profiles/r05/dense64_tile_ab.txt).  One MFMA is 2048 flop and occupies the DP pipe for tens of cycles,
// so one fragment value per operand per MFMA is far below what LDS delivers: the tile is sized by registers, not by
// LDS traffic.  Measured at N = 10003: 61.4 ms per propagation = 65.2 TF = 0.85 of the 77.2 TF the MFMA sustains.
// Kernel: 128 x 128 block tile, BK = 16, 4 waves each owning a 64 x 64 sub-tile = 4 x 4 accumulators of 16 x 16 (64 doubles
// = 128 accumulator registers per lane), two workgroups per CU.  Operands go global -> registers -> LDS, double-buffered
// (the next K tile's global loads fly under the MFMAs, one barrier per K tile); LDS images are [k][i] with strides that
// are odd in units of the store width (transposing b64 stores of A and of a k-contiguous B; b128 stores of a row-major B).
// Matrices are ld x ld with ld a multiple of 128 and zero padding, so no tile is ragged.
#include <hip/hip_runtime.h>

#include "ekf_dense.hpp"

namespace ekf {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

constexpr int BK64 = 16;
constexpr int kBig64 = 128;     // main kernel tile (square)
constexpr int kSmall64 = 64;    // tail kernel tile: a quarter of a main tile

// Tile id -> (tm, tn) in units of 128: the list is walked in groups of GROUP_M tile rows so that neighbouring tiles re-use
// their A and B panels out of L2 (speed only; the same order as ekf_dense.hip's big_tile_of).
__host__ __device__ inline void tile64_of(int id, int tiles, int& tm, int& tn) {
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * tiles;
    const int g = id / per_group;
    const int first_m = g * GROUP_M;
    const int gm = (tiles - first_m) < GROUP_M ? (tiles - first_m) : GROUP_M;
    const int in_g = id % per_group;
    tm = first_m + in_g % gm;
    tn = in_g / gm;
}

// How one product is cut: the (ld/128)^2 list of 128 x 128 tiles runs as whole rounds of resident workgroups on the main
// kernel (ids [0, n_big)); the rest of the list (n_small tiles) runs on the tail kernel behind it, each tile as four
// 64 x 64 quarters.
struct Dense64Split {
    int ld, tiles, n_big, n_small;
    int n_rows;   // rows of C that are not padding (N): the K loop stops there, and quarter tiles wholly below it are skipped
                  // (their rows of C are products of A's zero padding and stay the zeros they were allocated as)
};

// One output tile of (32*WTM) x (32*WTN): 4 waves as 2 x 2, each owning WTM x WTN accumulators of 16 x 16.
// NBUF = 2: double-buffered LDS, one barrier per K tile; NBUF = 1: one buffer, two barriers per K tile.
template <bool BT, int NBUF, int WTM, int WTN>
__device__ __forceinline__ void gemm64_tile(const double* __restrict__ A, const double* __restrict__ B,
                                            double* __restrict__ C, const double* __restrict__ Qadd, int ld, int row0,
                                            int col0, double* smem, int kdim) {
    constexpr int TM = 32 * WTM, TN = 32 * WTN;
    constexpr int SA = TM + 1;               // b64 transposing stores: odd stride in doubles
    constexpr int SB = BT ? TN + 1 : TN + 2; // a row-major B is copied with b128 stores: odd stride in 16-B units
    constexpr int A_ELEMS = (BK64 * SA + 1) / 2 * 2;   // keeps the B image 16-B aligned
    constexpr int B_ELEMS = BK64 * SB;
    constexpr int BUF_ELEMS = (A_ELEMS + B_ELEMS + 1) / 2 * 2;
    constexpr int PA = TM / 32;              // A staging passes: 32 rows x 16 k per pass (8 lanes x 16 B per row)
    constexpr int PBT = TN / 32;             // transposed-B staging passes
    constexpr int RB = 512 / TN;             // row-major B: k rows per pass (256 lanes x 2 doubles)
    constexpr int PB = BK64 / RB;
    static_assert(PA >= 1 && PBT >= 1 && PB >= 1, "tile too small for 256 threads");

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 15, lk = lane >> 4;
    const double* Ag = A + (size_t)row0 * ld;
    const double* Bg = BT ? B + (size_t)col0 * ld : B + col0;

    f64x2 ra[PA], rb[BT ? PBT : PB];
    auto gload = [&](int k0) {
#pragma unroll
        for (int p = 0; p < PA; p++) {
            const int row = p * 32 + (t >> 3), k2 = (t & 7) * 2;
            ra[p] = *reinterpret_cast<const f64x2*>(Ag + (size_t)row * ld + k0 + k2);
        }
        if constexpr (BT) {
#pragma unroll
            for (int p = 0; p < PBT; p++) {
                const int row = p * 32 + (t >> 3), k2 = (t & 7) * 2;
                rb[p] = *reinterpret_cast<const f64x2*>(Bg + (size_t)row * ld + k0 + k2);
            }
        } else {
#pragma unroll
            for (int p = 0; p < PB; p++) {
                const int k = p * RB + t / (TN / 2), j2 = (t % (TN / 2)) * 2;
                rb[p] = *reinterpret_cast<const f64x2*>(Bg + (size_t)(k0 + k) * ld + j2);
            }
        }
    };
    auto lstore = [&](int buf) {
        double* as = smem + buf * BUF_ELEMS;
        double* bs = as + A_ELEMS;
#pragma unroll
        for (int p = 0; p < PA; p++) {
            const int row = p * 32 + (t >> 3), k2 = (t & 7) * 2;
            as[k2 * SA + row] = ra[p][0];
            as[(k2 + 1) * SA + row] = ra[p][1];
        }
        if constexpr (BT) {
#pragma unroll
            for (int p = 0; p < PBT; p++) {
                const int row = p * 32 + (t >> 3), k2 = (t & 7) * 2;
                bs[k2 * SB + row] = rb[p][0];
                bs[(k2 + 1) * SB + row] = rb[p][1];
            }
        } else {
#pragma unroll
            for (int p = 0; p < PB; p++) {
                const int k = p * RB + t / (TN / 2), j2 = (t % (TN / 2)) * 2;
                *reinterpret_cast<f64x2*>(bs + k * SB + j2) = rb[p];
            }
        }
    };

    f64x4 acc[WTM][WTN];
#pragma unroll
    for (int i = 0; i < WTM; i++)
#pragma unroll
        for (int j = 0; j < WTN; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[i][j][r] = 0.0;

    const int nk = (kdim + BK64 - 1) / BK64;   // the K range behind N is zero padding in both operands
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int cur = NBUF == 2 ? (kt & 1) : 0;
        if (kt + 1 < nk) gload((kt + 1) * BK64);   // next tile's global loads fly under this tile's MFMAs
        // A operand of v_mfma_f64_16x16x4_f64: lane l holds A[i = l & 15][k = l >> 4]; B: B[k = l >> 4][j = l & 15]
        const double* as = smem + cur * BUF_ELEMS + wm * 16 * WTM + li;
        const double* bs = smem + cur * BUF_ELEMS + A_ELEMS + wn * 16 * WTN + li;
        double a[WTM], b[WTN];
#pragma unroll
        for (int i = 0; i < WTM; i++) a[i] = as[lk * SA + 16 * i];
#pragma unroll
        for (int j = 0; j < WTN; j++) b[j] = bs[lk * SB + 16 * j];
#pragma unroll
        for (int kk = 0; kk < BK64; kk += 4) {
            // fragments of k-step kk+4 are read before the MFMAs of k-step kk issue, so the reads hide under them
            double an[WTM], bn[WTN];
#pragma unroll
            for (int i = 0; i < WTM; i++) an[i] = 0.0;
#pragma unroll
            for (int j = 0; j < WTN; j++) bn[j] = 0.0;
            if (kk + 4 < BK64) {
#pragma unroll
                for (int i = 0; i < WTM; i++) an[i] = as[(kk + 4 + lk) * SA + 16 * i];
#pragma unroll
                for (int j = 0; j < WTN; j++) bn[j] = bs[(kk + 4 + lk) * SB + 16 * j];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < WTM; i++)
#pragma unroll
                for (int j = 0; j < WTN; j++)
                    acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < WTM; i++) a[i] = an[i];
#pragma unroll
            for (int j = 0; j < WTN; j++) b[j] = bn[j];
        }
        if (kt + 1 < nk) {
            if constexpr (NBUF == 2) {
                lstore(cur ^ 1);   // the other buffer was last read one barrier ago
                __syncthreads();
            } else {
                __syncthreads();   // every wave is done reading the only buffer
                lstore(0);
                __syncthreads();
            }
        }
    }

    // C/D map of v_mfma_f64_16x16x4_f64 (NOT the f32 16x16x4 map): col = lane & 15, row = (lane >> 4) + 4 * reg
    double* Cg = C + (size_t)(row0 + wm * 16 * WTM) * ld + col0 + wn * 16 * WTN;
    const double* Qg = Qadd ? Qadd + (size_t)(row0 + wm * 16 * WTM) * ld + col0 + wn * 16 * WTN : nullptr;
#pragma unroll
    for (int i = 0; i < WTM; i++)
#pragma unroll
        for (int j = 0; j < WTN; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int row = i * 16 + lk + 4 * r;
                const int col = j * 16 + li;
                double v = acc[i][j][r];
                if (Qg) v += Qg[(size_t)row * ld + col];
                Cg[(size_t)row * ld + col] = v;
            }
}

template <bool BT>
__global__ __launch_bounds__(256, 2) void k_gemm_f64_big(const double* __restrict__ A, const double* __restrict__ B,
                                                         double* __restrict__ C, const double* __restrict__ Qadd,
                                                         Dense64Split sp) {
    extern __shared__ __attribute__((aligned(16))) double smem64[];
    // consecutive workgroup ids are dealt round-robin to the 8 XCDs: remapped so that every XCD owns a contiguous chunk of
    // the grouped tile list and re-uses its panels out of its own L2
    int id = blockIdx.x;
    if (sp.n_big % 8 == 0) id = (id % 8) * (sp.n_big / 8) + id / 8;
    int tm, tn;
    tile64_of(id, sp.tiles, tm, tn);
    gemm64_tile<BT, 2, 4, 4>(A, B, C, Qadd, sp.ld, tm * kBig64, tn * kBig64, smem64, sp.n_rows);
}

template <bool BT>
__global__ __launch_bounds__(256, 4) void k_gemm_f64_tail(const double* __restrict__ A, const double* __restrict__ B,
                                                          double* __restrict__ C, const double* __restrict__ Qadd,
                                                          Dense64Split sp) {
    extern __shared__ __attribute__((aligned(16))) double smem64[];
    const int s = blockIdx.x;
    int tm, tn;
    tile64_of(sp.n_big + (s >> 2), sp.tiles, tm, tn);
    const int row0 = tm * kBig64 + ((s >> 1) & 1) * kSmall64;
    if (row0 >= sp.n_rows) return;   // (uniform) padding rows only
    gemm64_tile<BT, 1, 2, 2>(A, B, C, Qadd, sp.ld, row0, tn * kBig64 + (s & 1) * kSmall64, smem64, sp.n_rows);
}

static size_t lds64_bytes(int tm, int tn, bool bt, int nbuf) {
    const int a = (BK64 * (tm + 1) + 1) / 2 * 2, b = BK64 * (bt ? tn + 1 : tn + 2);
    return (size_t)nbuf * ((a + b + 1) / 2 * 2) * sizeof(double);
}

hipError_t dense64_gemm_prepare() {
    // the main kernel's two buffers take 64.8 KiB per workgroup: above the 48 KB a kernel may take without asking
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_f64_big<true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)lds64_bytes(kBig64, kBig64, true, 2));
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_f64_big<false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds64_bytes(kBig64, kBig64, false, 2));
}

static Dense64Split make_split64(int ld, int n_rows = 0) {
    Dense64Split sp{};
    sp.ld = ld;
    sp.n_rows = n_rows > 0 ? n_rows : ld;
    sp.tiles = ld / kBig64;
    const int total = sp.tiles * sp.tiles;
    const int slots = 256 * 2;   // resident workgroups: __launch_bounds__ of k_gemm_f64_big on 256 CUs
    int n_big = total / slots * slots;
    if (n_big == 0) n_big = total;   // (less than one round: all of it on the main kernel)
    sp.n_big = n_big;
    sp.n_small = total - n_big;
    return sp;
}

void dense64_gemm_split(int ld, int* tiles_out, int* n_big_out, int* n_rem_out) {
    const Dense64Split sp = make_split64(ld);
    if (tiles_out) *tiles_out = sp.tiles;
    if (n_big_out) *n_big_out = sp.n_big;
    if (n_rem_out) *n_rem_out = sp.n_small;
}

void dense64_gemm_tile_map(int ld, unsigned char* map) {
    const Dense64Split sp = make_split64(ld);
    const int t = sp.tiles;
    for (int i = 0; i < t * t; i++) map[i] = 255;
    for (int id = 0; id < sp.n_big + sp.n_small; id++) {   // (the XCD remap permutes ids inside [0, n_big) only)
        int tm, tn;
        tile64_of(id, t, tm, tn);
        map[tm * t + tn] = id < sp.n_big ? 0 : 1;
    }
}

void launch_dense64_gemm(const double* A, const double* B, double* C, const double* Qadd, int ld, bool b_transposed,
                         hipStream_t s, int n_rows) {
    const Dense64Split sp = make_split64(ld, n_rows);
    if (sp.n_big > 0) {
        const size_t lds = lds64_bytes(kBig64, kBig64, b_transposed, 2);
        if (b_transposed) hipLaunchKernelGGL((k_gemm_f64_big<true>), dim3(sp.n_big), dim3(256), lds, s, A, B, C, Qadd, sp);
        else hipLaunchKernelGGL((k_gemm_f64_big<false>), dim3(sp.n_big), dim3(256), lds, s, A, B, C, Qadd, sp);
    }
    if (sp.n_small > 0) {   // behind the main kernel on the same stream
        const size_t lds = lds64_bytes(kSmall64, kSmall64, b_transposed, 1);
        if (b_transposed) hipLaunchKernelGGL((k_gemm_f64_tail<true>), dim3(4 * sp.n_small), dim3(256), lds, s, A, B, C, Qadd, sp);
        else hipLaunchKernelGGL((k_gemm_f64_tail<false>), dim3(4 * sp.n_small), dim3(256), lds, s, A, B, C, Qadd, sp);
    }
}

}  // namespace ekf
