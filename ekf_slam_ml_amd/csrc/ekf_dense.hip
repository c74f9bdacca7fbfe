// ekf_dense.hip -- dense general-F covariance propagation Sigma <- F * Sigma * F^T + Q on the gfx950 matrix cores, fp32 and
// fp64: the one translation unit that instantiates the kernels of ekf_dense_gemm.hpp for both element types, and the host
// side that ekf_dense.hpp declares -- the launcher, the report of the split and the LDS-limit set-up.
#include "ekf_dense.hpp"
#include "ekf_dense_gemm.hpp"

namespace ekf {

template <class E>
hipError_t dense_gemm_prepare() {
    // the main kernels stage 49.4 KB (fp32) and 64.8 KiB (fp64) per workgroup: above the 48 KB a kernel may take without asking
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_big<E, true>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)GemmMainTile<E, true>::kLdsBytes);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&k_gemm_big<E, false>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)GemmMainTile<E, false>::kLdsBytes);
}

template <class E>
void dense_gemm_split(int ld, int* tiles_out, int* n_big_out, int* n_rem_out) {
    const DenseSplit sp = make_split<E>(ld);
    if (tiles_out) *tiles_out = sp.tiles_n;
    if (n_big_out) *n_big_out = sp.n_big;
    if (n_rem_out) *n_rem_out = sp.n_small;
}

template <class E>
void dense_gemm_tile_map(int ld, unsigned char* map) {
    dense_tile_map<E>(make_split<E>(ld), map);
}

template <class E, bool BT>
static void launch(const E* A, const E* B, E* C, const E* Qadd, const DenseSplit& sp, hipStream_t s) {
    constexpr size_t lds_big = GemmMainTile<E, BT>::kLdsBytes, lds_tail = GemmTailTile<E, BT>::kLdsBytes;
    if (sp.n_big > 0) hipLaunchKernelGGL((k_gemm_big<E, BT>), dim3(sp.n_big), dim3(256), lds_big, s, A, B, C, Qadd, sp);
    if (sp.n_small > 0)   // behind the main kernel on the same stream (see k_gemm_big)
        hipLaunchKernelGGL((k_gemm_tail<E, BT>), dim3(4 * sp.n_small), dim3(256), lds_tail, s, A, B, C, Qadd, sp);
}

template <class E>
void launch_dense_gemm(const E* A, const E* B, E* C, const E* Qadd, int ld, bool b_transposed, hipStream_t s, int n_rows) {
    const DenseSplit sp = make_split<E>(ld, n_rows);
    if (b_transposed) launch<E, true>(A, B, C, Qadd, sp, s);
    else launch<E, false>(A, B, C, Qadd, sp, s);
}

#define EKF_DENSE_INSTANTIATE(E)                                                                                  \
    template hipError_t dense_gemm_prepare<E>();                                                                  \
    template void dense_gemm_split<E>(int, int*, int*, int*);                                                     \
    template void dense_gemm_tile_map<E>(int, unsigned char*);                                                    \
    template void launch_dense_gemm<E>(const E*, const E*, E*, const E*, int, bool, hipStream_t, int);
EKF_DENSE_INSTANTIATE(float)
EKF_DENSE_INSTANTIATE(double)
#undef EKF_DENSE_INSTANTIATE

}  // namespace ekf
