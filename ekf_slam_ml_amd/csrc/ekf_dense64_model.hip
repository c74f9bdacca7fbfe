// ekf_dense64_model.hip -- the reference's motion model and the top of its measurement() on the dense64 handle's own state
// (gfx950, wave64): what a caller of the model-free propagate_block would otherwise read the heading back for.
//   k_dmd_predict   one thread: Fr = I + A (3 x 3), Qr = q_pose I and dx of prediction() (:67-96) from state[0] and the twist,
//                   written where ekf_dense64_propagate_block's uploads go
//   k_dmd_snapshot  the pose state[0..2] into a slot of its own (:109-111): measurement() captures it once per call
//   k_dmd_init      one thread per landmark: state[3 + 2 i .. 4 + 2 i] from reading i and the snapshot pose (:114-125)
// No atomics, no LDS; the model itself is ekf_kernels.hpp's (motion_terms, landmark_from_reading), not a second copy.
#include "ekf_dense.hpp"
#include "ekf_kernels.hpp"

namespace ekf {
namespace {

constexpr int kModelThreads = 256;

// two doubles that sit on an 8-byte boundary only (landmark i starts at state + 3 + 2 i): one 16-byte access
typedef double pair8 __attribute__((ext_vector_type(2), aligned(8)));
typedef double pair16 __attribute__((ext_vector_type(2)));

__global__ void k_dmd_predict(const double* __restrict__ state, double dtheta, double dx, double q_pose,
                              double straight_eps, double* __restrict__ Fr, double* __restrict__ Qr,
                              double* __restrict__ upd) {
    if (threadIdx.x != 0) return;
    MotionTerms m;
    motion_terms(state[0], dtheta, dx, straight_eps, m);
    // At = eye + A (:101): the identity except (1,0) and (2,0)
    Fr[0] = 1.0; Fr[1] = 0.0; Fr[2] = 0.0;
    Fr[3] = 0.0 + m.a10; Fr[4] = 1.0; Fr[5] = 0.0;
    Fr[6] = 0.0 + m.a20; Fr[7] = 0.0; Fr[8] = 1.0;
#pragma unroll
    for (int k = 0; k < 9; k++) Qr[k] = (k % 4 == 0) ? q_pose : 0.0;   // :40-43
    upd[0] = m.upd[0]; upd[1] = m.upd[1]; upd[2] = m.upd[2];
}

__global__ void k_dmd_snapshot(const double* __restrict__ state, double* __restrict__ pose) {
    if (threadIdx.x < 3) pose[threadIdx.x] = state[threadIdx.x];
}

__global__ __launch_bounds__(kModelThreads) void k_dmd_init(const double* __restrict__ pose,
                                                            const double* __restrict__ sensor_xy, int n_lm,
                                                            double* __restrict__ state) {
    const int i = blockIdx.x * kModelThreads + threadIdx.x;
    if (i >= n_lm) return;
    const double theta = pose[0], x = pose[1], y = pose[2];
    const pair16 z = reinterpret_cast<const pair16*>(sensor_xy)[i];
    double mx, my;
    landmark_from_reading(z.x, z.y, theta, x, y, mx, my);
    *reinterpret_cast<pair8*>(state + 3 + 2 * (size_t)i) = pair8{mx, my};
}

}  // namespace

void launch_dense64_model_predict(const double* state, double dtheta, double dx, double q_pose, double straight_eps,
                                  double* Fr, double* Qr, double* upd, hipStream_t st) {
    hipLaunchKernelGGL(k_dmd_predict, dim3(1), dim3(64), 0, st, state, dtheta, dx, q_pose, straight_eps, Fr, Qr, upd);
}

void launch_dense64_model_snapshot(const double* state, double* pose, hipStream_t st) {
    hipLaunchKernelGGL(k_dmd_snapshot, dim3(1), dim3(64), 0, st, state, pose);
}

void launch_dense64_model_init(const double* pose, const double* sensor_xy, int n_lm, double* state, hipStream_t st) {
    hipLaunchKernelGGL(k_dmd_init, dim3((n_lm + kModelThreads - 1) / kModelThreads), dim3(kModelThreads), 0, st, pose,
                       sensor_xy, n_lm, state);
}

}  // namespace ekf
