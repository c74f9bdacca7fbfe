// ekf_capi_dense.hip -- C ABI of include/ekfslam.h, dense general-F covariance propagation: the fp32 handle (configs[3])
// and what its fp64 twin shares with it.  create, destroy, set, propagate, get_sigma, launch_info and tile_map of the two
// handles are one template over the element type, and so are the kernels behind them (ekf_dense.hip); what a
// handle owns beyond Sigma it sets up, releases and keeps consistent in the hooks of ekf_dense_handle.hpp.  Everything else
// the fp64 handle can do is in ekf_capi_dense64.hip.
#include "ekf_dense_handle.hpp"

using namespace ekfrt;

namespace {

// the element type of a handle: what picks the instantiation of the launcher, the split report and the LDS-limit set-up
template <class H> using elem_t = std::remove_pointer_t<decltype(H::F)>;

template <class H>
ekf_status dense_destroy(H* d) {
    if (!d) return EKF_OK;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    d->mem.free_all();
    d->destroying();
    for (hipEvent_t e : {d->e0, d->e1})
        if (e) (void)hipEventDestroy(e);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
    return EKF_OK;
}

template <class H>
ekf_status dense_create(const char* name, int N, int device, H** out) {
    if (!out || N <= 0) return fail(EKF_ERR_INVALID, std::string(name) + ": bad argument");
    *out = nullptr;
    EKFC(select_device(&device, true));
    H* d = new (std::nothrow) H();
    if (!d) return fail(EKF_ERR_NOMEM, "host allocation failed");
    d->device = device;
    d->N = N;
    d->ld = round_up(N, ekf::kDenseTile);
    ekf_status st = EKF_OK;
    auto body = [&]() -> ekf_status {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        d->mem.stream = d->stream;
        HIPC(ekf::dense_gemm_prepare<elem_t<H>>());
        for (auto** p : {&d->F, &d->S, &d->T, &d->Q}) EKFC(d->mem.alloc(p, (size_t)d->ld * d->ld, Fill::kZero, name, "the matrices"));
        EKFC(d->created());
        HIPC(hipEventCreate(&d->e0));
        HIPC(hipEventCreate(&d->e1));
        HIPC(hipStreamSynchronize(d->stream));
        return EKF_OK;
    };
    st = body();
    if (st != EKF_OK) {
        dense_destroy(d);
        return st;
    }
    *out = d;
    return EKF_OK;
}

template <class H, class E>
ekf_status dense_set(H* d, const E* F, const E* Sigma, const E* Q) {
    if (!d) return fail(EKF_ERR_INVALID, "null handle");
    HIPC(hipSetDevice(d->device));
    const size_t w = sizeof(E) * d->N, pitch = sizeof(E) * d->ld;
    const E* src[3] = {F, Sigma, Q};
    E* dst[3] = {d->F, d->S, d->Q};
    for (int i = 0; i < 3; i++)
        if (src[i]) HIPC(hipMemcpy2DAsync(dst[i], pitch, src[i], w, w, d->N, hipMemcpyHostToDevice, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    if (Sigma) d->sigma_replaced();
    return EKF_OK;
}

template <class H>
ekf_status dense_propagate(const char* name, H* d, int iterations, double* elapsed_ms) {
    if (!d || iterations < 0) return fail(EKF_ERR_INVALID, std::string(name) + ": bad argument");
    HIPC(hipSetDevice(d->device));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->sigma_needed();
    for (int it = 0; it < iterations; it++) {
        ekf::launch_dense_gemm<elem_t<H>>(d->F, d->S, d->T, nullptr, d->ld, false, d->stream, d->N);  // T = At*sigma (:102)
        ekf::launch_dense_gemm<elem_t<H>>(d->T, d->F, d->S, d->Q, d->ld, true, d->stream, d->N);      // sigma = T*At.t() + Q
    }
    return finish_timed(d, elapsed_ms);
}

template <class H>
ekf_status dense_launch_info(H* d, int* ld, int* tiles, int* n_big, int* n_tail) {
    if (!d) return fail(EKF_ERR_INVALID, "null handle");
    if (ld) *ld = d->ld;
    ekf::dense_gemm_split<elem_t<H>>(d->ld, tiles, n_big, n_tail);
    return EKF_OK;
}

template <class H>
ekf_status dense_tile_map(H* d, unsigned char* map) {
    if (!d || !map) return fail(EKF_ERR_INVALID, "null argument");
    ekf::dense_gemm_tile_map<elem_t<H>>(d->ld, map);
    return EKF_OK;
}

template <class H, class E>
ekf_status dense_get_sigma(H* d, E* out) {
    if (!d || !out) return fail(EKF_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(d->device));
    d->sigma_needed();
    const size_t w = sizeof(E) * d->N, pitch = sizeof(E) * d->ld;
    HIPC(hipMemcpy2DAsync(out, w, d->S, pitch, w, d->N, hipMemcpyDeviceToHost, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}

}  // namespace

extern "C" {

ekf_status ekf_dense_create(int N, int device, ekf_dense_handle* out) {
    return dense_create<ekf_dense_s>("ekf_dense_create", N, device, out);
}
ekf_status ekf_dense_destroy(ekf_dense_handle d) { return dense_destroy(d); }
ekf_status ekf_dense_set(ekf_dense_handle d, const float* F, const float* Sigma, const float* Q) {
    return dense_set(d, F, Sigma, Q);
}
ekf_status ekf_dense_propagate(ekf_dense_handle d, int iterations, double* elapsed_ms) {
    return dense_propagate("ekf_dense_propagate", d, iterations, elapsed_ms);
}
ekf_status ekf_dense_launch_info(ekf_dense_handle d, int* ld, int* tiles, int* n_big, int* n_tail) {
    return dense_launch_info(d, ld, tiles, n_big, n_tail);
}
ekf_status ekf_dense_tile_map(ekf_dense_handle d, unsigned char* map) { return dense_tile_map(d, map); }
ekf_status ekf_dense_get_sigma(ekf_dense_handle d, float* out) { return dense_get_sigma(d, out); }

ekf_status ekf_dense64_create(int N, int device, ekf_dense64_handle* out) {
    return dense_create<ekf_dense64_s>("ekf_dense64_create", N, device, out);
}
ekf_status ekf_dense64_destroy(ekf_dense64_handle d) { return dense_destroy(d); }
ekf_status ekf_dense64_set(ekf_dense64_handle d, const double* F, const double* Sigma, const double* Q) {
    if (d) d->leave_region();   // outside a region's terms: it ends first
    return dense_set(d, F, Sigma, Q);
}
ekf_status ekf_dense64_propagate(ekf_dense64_handle d, int iterations, double* elapsed_ms) {
    return dense_propagate("ekf_dense64_propagate", d, iterations, elapsed_ms);
}
ekf_status ekf_dense64_launch_info(ekf_dense64_handle d, int* ld, int* tiles, int* n_big, int* n_tail) {
    return dense_launch_info(d, ld, tiles, n_big, n_tail);
}
ekf_status ekf_dense64_tile_map(ekf_dense64_handle d, unsigned char* map) { return dense_tile_map(d, map); }
ekf_status ekf_dense64_get_sigma(ekf_dense64_handle d, double* out) { return dense_get_sigma(d, out); }

}  // extern "C"
