// A/B of the fp64 tile for the dense propagation (ekf_dense_gemm.hpp, instantiated in ekf_dense.hip): the same 128 x 128 x 16 block tile, 256 threads,
// double-buffered LDS, grouped tile order, one product C = A * B (NN) at N = 10003 (ld = 10112), built two ways:
//   M  the product's k_gemm_big<double>: 4 waves x (4 x 4) v_mfma_f64_16x16x4_f64 accumulators
//   V  register-blocked v_fma_f64: every thread owns an 8 x 8 block of C (rows / columns 32 c + 2 t + e), operands read
//      from LDS as b128 pairs, 64 explicit fma() per k (the library is built with -ffp-contract=off)
// Both run the whole tile list in ONE launch of 6241 workgroups (12.2 rounds of 512 resident), so they differ in the
// inner product only; the product's own launch path (main kernel in whole rounds + quarter-tile tail) is timed as "P".
// Outputs are compared (fp64 both: only the summation order differs).
// The ceilings the shares are taken against come from the same process: each instruction issued back to back on 16
// independent accumulators with constant operands, 512 workgroups of 256 threads (two waves per SIMD, as the GEMMs).
// (tools/micro/mfma_f64_peak.hip's 46 TF feeds at most 4 accumulators and adds a v_add_f64 to the operand every
// iteration: it is no ceiling for a tile that keeps 16 accumulators in flight.)
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 -o tools/micro/dense64_tile_ab tools/micro/dense64_tile_ab.hip
#include "../../ekf_slam_ml_amd/csrc/ekf_dense.hip"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#define CK(x)                                                                           \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) {                                                         \
            std::printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__);  \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

namespace {
using ekf::f64x2;
constexpr int BK = ekf::GemmMainTile<double, false>::BK;
constexpr int S = 130;   // LDS row stride in doubles: odd in 16-B units
constexpr int BUF = 2 * BK * S;

__global__ __launch_bounds__(256, 2) void k_valu(const double* __restrict__ A, const double* __restrict__ B,
                                                 double* __restrict__ C, int ld, int kdim, int tiles) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    int tm, tn;
    ekf::big_tile_of(blockIdx.x, tiles, tiles, tm, tn);
    const int row0 = tm * 128, col0 = tn * 128;
    const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
    const double* Ag = A + (size_t)row0 * ld;
    const double* Bg = B + col0;
    f64x2 ra[4], rb[4];
    auto gload = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = p * 32 + (t >> 3), k2 = (t & 7) * 2;
            ra[p] = *reinterpret_cast<const f64x2*>(Ag + (size_t)row * ld + k0 + k2);
            const int k = p * 4 + (t >> 6), j2 = (t & 63) * 2;
            rb[p] = *reinterpret_cast<const f64x2*>(Bg + (size_t)(k0 + k) * ld + j2);
        }
    };
    auto lstore = [&](int buf) {
        double* as = sm + buf * BUF;
        double* bs = as + BK * S;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int row = p * 32 + (t >> 3), k2 = (t & 7) * 2;
            as[k2 * S + row] = ra[p][0];
            as[(k2 + 1) * S + row] = ra[p][1];
            const int k = p * 4 + (t >> 6), j2 = (t & 63) * 2;
            *reinterpret_cast<f64x2*>(bs + k * S + j2) = rb[p];
        }
    };
    double acc[8][8];
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) acc[i][j] = 0.0;
    const int nk = (kdim + BK - 1) / BK;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kt = 0; kt < nk; kt++) {
        const int cur = kt & 1;
        if (kt + 1 < nk) gload((kt + 1) * BK);
        const double* as = sm + cur * BUF + 2 * ty;
        const double* bs = sm + cur * BUF + BK * S + 2 * tx;
#pragma unroll 4
        for (int k = 0; k < BK; k++) {
            double a[8], b[8];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const f64x2 va = *reinterpret_cast<const f64x2*>(as + k * S + 32 * c);
                const f64x2 vb = *reinterpret_cast<const f64x2*>(bs + k * S + 32 * c);
                a[2 * c] = va[0]; a[2 * c + 1] = va[1];
                b[2 * c] = vb[0]; b[2 * c + 1] = vb[1];
            }
#pragma unroll
            for (int i = 0; i < 8; i++)
#pragma unroll
                for (int j = 0; j < 8; j++) acc[i][j] = __builtin_fma(a[i], b[j], acc[i][j]);
        }
        if (kt + 1 < nk) {
            lstore(cur ^ 1);
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int row = row0 + 32 * (i >> 1) + 2 * ty + (i & 1);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int col = col0 + 32 * c + 2 * tx;
            *reinterpret_cast<f64x2*>(C + (size_t)row * ld + col) = f64x2{acc[i][2 * c], acc[i][2 * c + 1]};
        }
    }
}

template <int NACC>
__global__ __launch_bounds__(256, 2) void k_mfma_ceiling(double* out, int iters) {
    typedef double d4 __attribute__((ext_vector_type(4)));
    d4 acc[NACC];
    for (int i = 0; i < NACC; i++) acc[i] = d4{0.0, 0.0, 0.0, 0.0};
    const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < NACC; i++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0;
    for (int i = 0; i < NACC; i++) s += acc[i].x + acc[i].y + acc[i].z + acc[i].w;
    out[blockIdx.x * 256 + threadIdx.x] = s;
}
template <int NACC>
__global__ __launch_bounds__(256, 2) void k_fma_ceiling(double* out, int iters) {
    double x[NACC];
    for (int i = 0; i < NACC; i++) x[i] = 1.0 + i * 1e-3;
    const double m = 1.0 - threadIdx.x * 1e-12, c = 1e-9;
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int i = 0; i < NACC; i++) x[i] = __builtin_fma(x[i], m, c);
    }
    double s = 0;
    for (int i = 0; i < NACC; i++) s += x[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

// deterministic values in [-1, 1) inside the N x N corner, zero padding outside
__global__ void k_fill(double* X, int ld, int N, unsigned seed) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)ld * ld) return;
    const int r = (int)(i / ld), c = (int)(i % ld);
    unsigned h = (unsigned)i * 2654435761u ^ seed;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    X[i] = (r < N && c < N) ? (double)(h & 0xFFFFF) / 524288.0 - 1.0 : 0.0;
}
}  // namespace

int main(int argc, char** argv) {
    const int N = argc > 1 ? std::atoi(argv[1]) : 10003;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
    const int ld = (N + 127) / 128 * 128, tiles = ld / 128;
    const size_t bytes = sizeof(double) * (size_t)ld * ld;
    double *A, *B, *CM, *CV;
    CK(hipMalloc(&A, bytes)); CK(hipMalloc(&B, bytes)); CK(hipMalloc(&CM, bytes)); CK(hipMalloc(&CV, bytes));
    CK(hipMemset(CM, 0, bytes)); CK(hipMemset(CV, 0, bytes));
    const unsigned fb = (unsigned)(((size_t)ld * ld + 255) / 256);
    hipLaunchKernelGGL(k_fill, dim3(fb), dim3(256), 0, 0, A, ld, N, 1u);
    hipLaunchKernelGGL(k_fill, dim3(fb), dim3(256), 0, 0, B, ld, N, 2u);
    CK(ekf::dense_gemm_prepare<double>());
    const size_t lds_m = ekf::GemmMainTile<double, false>::kLdsBytes, lds_v = sizeof(double) * 2 * BUF;
    CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_valu), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_v));
    ekf::DenseSplit one{};   // the whole tile list on one launch of the main kernel (no XCD remap: 6241 % 8 != 0)
    one.ld = ld; one.tiles_m = one.tiles_n = tiles; one.n_big = tiles * tiles; one.n_rows = N;
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    auto timed = [&](int which) -> float {
        hipEventRecord(e0, 0);
        if (which == 0) hipLaunchKernelGGL((ekf::k_gemm_big<double, false>), dim3(one.n_big), dim3(256), lds_m, 0, A, B, CM, nullptr, one);
        else if (which == 1) hipLaunchKernelGGL(k_valu, dim3(tiles * tiles), dim3(256), lds_v, 0, A, B, CV, ld, N, tiles);
        else ekf::launch_dense_gemm<double>(A, B, CM, nullptr, ld, false, 0, N);
        hipEventRecord(e1, 0);
        hipEventSynchronize(e1);
        float ms = 0.f;
        hipEventElapsedTime(&ms, e0, e1);
        return ms;
    };
    std::vector<float> t[3];
    for (int w = 0; w < 2; w++)
        for (int f = 0; f < 3; f++) timed(f);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    for (int r = 0; r < reps; r++)
        for (int f = 0; f < 3; f++) t[f].push_back(timed(f));
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    // outputs: M (last written by P, the same products) against V
    std::vector<double> hm((size_t)ld * ld), hv((size_t)ld * ld);
    CK(hipMemcpy(hm.data(), CM, bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(hv.data(), CV, bytes, hipMemcpyDeviceToHost));
    double dmax = 0, cmax = 0;
    for (size_t i = 0; i < hm.size(); i++) {
        dmax = std::max(dmax, std::fabs(hm[i] - hv[i]));
        cmax = std::max(cmax, std::fabs(hm[i]));
    }
    // instruction ceilings (same grid shape as the GEMMs: 512 workgroups x 256 threads)
    double tf_ceil[2] = {0, 0};
    {
        const int im = 40000, iv = 600000;
        for (int rep = 0; rep < 3; rep++) {
            hipEventRecord(e0, 0);
            hipLaunchKernelGGL(k_mfma_ceiling<16>, dim3(512), dim3(256), 0, 0, CV, im);
            hipEventRecord(e1, 0);
            hipEventSynchronize(e1);
            float ms = 0.f;
            hipEventElapsedTime(&ms, e0, e1);
            tf_ceil[0] = std::max(tf_ceil[0], 2048.0 * 16 * (double)im * 4 * 512 / (ms * 1e-3) / 1e12);
            hipEventRecord(e0, 0);
            hipLaunchKernelGGL(k_fma_ceiling<16>, dim3(512), dim3(256), 0, 0, CV, iv);
            hipEventRecord(e1, 0);
            hipEventSynchronize(e1);
            hipEventElapsedTime(&ms, e0, e1);
            tf_ceil[1] = std::max(tf_ceil[1], 2.0 * 16 * (double)iv * 256 * 512 / (ms * 1e-3) / 1e12);
        }
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        CK(hipMemset(CV, 0, bytes));
    }
    const double flop = 2.0 * N * (double)N * N;
    const char* name[3] = {"M  v_mfma_f64_16x16x4_f64, one launch", "V  v_fma_f64 8x8 per thread, one launch",
                           "P  product launch (main rounds + tail)"};
    std::printf("dense64 tile A/B: C = A * B (NN), N = %d, ld = %d, %d tiles of 128 x 128, %d timed each (alternating)\n",
                N, ld, tiles * tiles, reps);
    std::printf("ceilings (best of 3, 16 independent accumulators, 2 waves/SIMD): v_mfma_f64_16x16x4_f64 %.2f TF, "
                "v_fma_f64 %.2f TF\n", tf_ceil[0], tf_ceil[1]);
    for (int f = 0; f < 3; f++) {
        std::vector<float> s = t[f];
        std::sort(s.begin(), s.end());
        const float med = s[s.size() / 2];
        const double tf = flop / (med * 1e-3) / 1e12;
        std::printf("%-42s median %8.3f ms  min %8.3f ms  %6.2f TF algorithmic (2 N^3) = %.3f of its instruction's ceiling\n",
                    name[f], med, s[0], tf, tf / tf_ceil[f == 1 ? 1 : 0]);
    }
    std::printf("max |M - V| = %.3e (max |C| = %.3e): %s\n", dmax, cmax, dmax <= 1e-12 * cmax ? "agree" : "DISAGREE");
    return dmax <= 1e-12 * cmax ? 0 : 2;
}
