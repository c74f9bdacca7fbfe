// ekf_capi_sim.hip -- C ABI of include/ekfslam.h, on-device inputs and statistics: the simulator's logs and laser
// scans, the batched circle fitting, Monte-Carlo consistency.
#include "ekf_runtime.hpp"

using namespace ekfrt;

extern "C" {

void ekf_default_sim_params(ekf_sim_params* out) {
    if (!out) return;
    out->seed = 5000000ull;
    out->first_filter_id = 0;
    out->v_cmd = 0.5; out->w_cmd = 0.06;
    out->vx_std = 0.01; out->the_std = 0.01;      // noise_param.yaml:3,5
    out->slip_min = 0.90; out->slip_max = 1.10;   // noise_param.yaml:6-7
    out->sensor_std = 0.005;                      // noise_param.yaml:8-9
    out->max_visible_dis = 0.7;                   // noise_param.yaml:10
    out->wheel_base = 0.16; out->wheel_radius = 0.033;  // fake_turtle_param.yaml:6-7
    out->ticks_per_step = 10;
}

static ekf::SimParams to_sim(const ekf_sim_params* sp) {
    return ekf::SimParams{sp->seed, sp->first_filter_id, sp->v_cmd, sp->w_cmd, sp->vx_std, sp->the_std, sp->slip_min,
                          sp->slip_max, sp->sensor_std, sp->max_visible_dis, sp->wheel_base, sp->wheel_radius,
                          sp->ticks_per_step};
}

static bool lidar_ok(const ekf_lidar_params* lp) {
    return lp->n_beams >= 8 && lp->n_beams <= ekf::circles_max_beams() && lp->range_max > 0 && lp->border_width > 0 &&
           lp->tube_radius > 0 && lp->range_std >= 0 && (lp->model == 0 || (lp->model == 1 && lp->range_min > 0));
}

static ekf::LidarParams to_lidar(const ekf_lidar_params* lp) {
    return ekf::LidarParams{lp->n_beams, lp->range_std, lp->range_max, lp->border_width, lp->tube_radius, lp->model, lp->range_min};
}

ekf_status ekf_batch_simulate_known_log(ekf_batch_handle hb, const ekf_sim_params* sp, const double* world_xy, int T,
                                        int vmax) {
    if (!hb || !sp || !world_xy || T <= 0 || vmax < 0 || vmax > 64 || sp->ticks_per_step < 1)
        return fail(EKF_ERR_INVALID, "ekf_batch_simulate_known_log: bad argument (vmax <= 64)");
    Pool& P = hb->pool;
    EKFC(P.use());
    EKFC(free_log(P));
    const int B = P.pv.B, n = P.pv.n;
    const size_t n_tw = (size_t)T * B * 2, n_lm = (size_t)T * B * vmax, n_z = n_lm * 2, n_in = (size_t)B * 2 * n,
                 n_tr = (size_t)T * B * 3;
    const char* fn = "ekf_batch_simulate_known_log";
    EKFC(P.mem.replace_group({target(&P.log_twist, n_tw), target(&P.log_lm, n_lm ? n_lm : 1), target(&P.log_z, n_z ? n_z : 1),
                              target(&P.log_init, n_in ? n_in : 1), target(&P.log_truth, n_tr)}, fn, "the log"));
    ScopedMem tmp(P.stream);
    double* d_world = nullptr;
    int* d_active = nullptr;
    const size_t n_act = (size_t)T * (vmax > 0 ? vmax : 1);
    EKFC(tmp.replace_group({target(&d_world, (size_t)2 * (n > 0 ? n : 1)), target(&d_active, n_act, Fill::kZero)}, fn, "the world"));
    if (n > 0) HIPC(hipMemcpyAsync(d_world, world_xy, sizeof(double) * 2 * n, hipMemcpyHostToDevice, P.stream));
    ekf::launch_sim(to_sim(sp), B, n, T, vmax, d_world, P.log_twist, P.log_truth, P.log_lm, P.log_z, P.log_init, d_active,
                    P.stream);
    HIPC(hipGetLastError());
    std::vector<int> active(n_act, 0);
    HIPC(hipMemcpyAsync(active.data(), d_active, sizeof(int) * n_act, hipMemcpyDeviceToHost, P.stream));
    HIPC(hipStreamSynchronize(P.stream));
    P.slot_active.swap(active);
    std::vector<int> lm_host(n_lm ? n_lm : 1, -1);
    if (n_lm) HIPC(hipMemcpy(lm_host.data(), P.log_lm, sizeof(int) * n_lm, hipMemcpyDeviceToHost));
    P.compute_log_touch_bound(lm_host.data(), T, vmax);
    P.T = T;
    P.truth_is_unknown_log = 0;
    P.vmax = vmax;
    return EKF_OK;
}

ekf_status ekf_batch_download_log(ekf_batch_handle hb, double* twist, int* lm_idx, double* z_xy, double* init_xy,
                                  double* true_pose) {
    if (!hb) return fail(EKF_ERR_INVALID, "null handle");
    Pool& P = hb->pool;
    if (P.T <= 0) return fail(EKF_ERR_STATE, "no log on the device");
    if (true_pose && !P.log_truth) return fail(EKF_ERR_STATE, "the uploaded log carries no simulated truth");
    EKFC(P.use());
    HIPC(hipStreamSynchronize(P.stream));
    const size_t B = P.pv.B, T = P.T, vmax = P.vmax, n = P.pv.n;
    if (twist) HIPC(hipMemcpy(twist, P.log_twist, sizeof(double) * T * B * 2, hipMemcpyDeviceToHost));
    if (lm_idx && vmax) HIPC(hipMemcpy(lm_idx, P.log_lm, sizeof(int) * T * B * vmax, hipMemcpyDeviceToHost));
    if (z_xy && vmax) HIPC(hipMemcpy(z_xy, P.log_z, sizeof(double) * T * B * vmax * 2, hipMemcpyDeviceToHost));
    if (init_xy && n) HIPC(hipMemcpy(init_xy, P.log_init, sizeof(double) * B * 2 * n, hipMemcpyDeviceToHost));
    if (true_pose) HIPC(hipMemcpy(true_pose, P.log_truth, sizeof(double) * T * B * 3, hipMemcpyDeviceToHost));
    return EKF_OK;
}

ekf_status ekf_batch_mc_stats(ekf_batch_handle hb, int t, double out[6]) {
    if (!hb || !out) return fail(EKF_ERR_INVALID, "null argument");
    Pool& P = hb->pool;
    const double* truth = P.truth_is_unknown_log ? P.ulog_truth : P.log_truth;
    const int Tl = P.truth_is_unknown_log ? P.uT : P.T;
    if (!truth) return fail(EKF_ERR_STATE, "ekf_batch_mc_stats needs a simulated log (ground truth)");
    if (t < 0 || t >= Tl) return fail(EKF_ERR_INVALID, "step outside the log");
    EKFC(P.use());
    EKFC(P.flush());
    ekf::launch_mc_stats(P.pv, truth + (size_t)t * P.pv.B * 3, P.digest_dev, P.stream);
    EKFC(checked_launch());
    std::vector<double> h((size_t)4 * P.pv.B);
    EKFC(P.download(h.data(), P.digest_dev, sizeof(double) * h.size()));
    double nees = 0, nmax = 0, p2 = 0, a2 = 0, tr = 0, inside = 0;
    for (int b = 0; b < P.pv.B; b++) {
        const double v = h[(size_t)b * 4];
        nees += v; if (v > nmax) nmax = v;
        p2 += h[(size_t)b * 4 + 1]; a2 += h[(size_t)b * 4 + 2]; tr += h[(size_t)b * 4 + 3];
        if (v < 7.815) inside += 1.0;
    }
    const double Bn = (double)P.pv.B;
    out[0] = nees / Bn; out[1] = nmax; out[2] = std::sqrt(p2 / Bn); out[3] = std::sqrt(a2 / Bn); out[4] = tr / Bn;
    out[5] = inside / Bn;
    return EKF_OK;
}

void ekf_default_lidar_params(ekf_lidar_params* out) {
    if (!out) return;
    out->n_beams = 360;          // tube_world.cpp:452
    out->range_std = 0.005;      // noise_param.yaml
    out->range_max = 3.5;        // tube_world.cpp:476
    out->border_width = 2.0;     // tube_param.yaml
    out->tube_radius = 0.0762;   // tube_param.yaml
    out->model = 0;              // clean ray geometry (1: publishScan's own procedure)
    out->range_min = 0.12;       // tube_world.cpp:475
}

ekf_status ekf_batch_simulate_unknown_log(ekf_batch_handle hb, const ekf_sim_params* sp, const ekf_lidar_params* lidar,
                                          const double* world_xy, int T, int jmax) {
    if (!hb || !sp || !world_xy || T <= 0 || jmax < 1 || jmax > 64 || sp->ticks_per_step < 1 || (lidar && !lidar_ok(lidar)))
        return fail(EKF_ERR_INVALID, "ekf_batch_simulate_unknown_log: bad argument (1 <= jmax <= 64, 8 <= n_beams <= 1024)");
    Pool& P = hb->pool;
    EKFC(P.use());
    EKFC(free_ulog(P));
    const int B = P.pv.B, n = P.pv.n;
    const size_t n_tw = (size_t)T * B * 2, n_ct = (size_t)T * B, n_me = n_ct * jmax * 2, n_as = n_ct * jmax, n_tr = n_ct * 3;
    const char* fn = "ekf_batch_simulate_unknown_log";
    EKFC(P.mem.replace_group({target(&P.ulog_twist, n_tw), target(&P.ulog_count, n_ct), target(&P.ulog_meas, n_me, Fill::kZero),
                              target(&P.ulog_assoc, n_as, Fill::kOnes),   // -1; run_unknown overwrites
                              target(&P.ulog_truth, n_tr)}, fn, "the log"));
    if (!P.corr_counter) EKFC(P.dalloc(&P.corr_counter, 1));
    ScopedMem tmp(P.stream);
    double *d_world = nullptr, *d_ranges = nullptr, *d_radii = nullptr;
    EKFC(tmp.alloc(&d_world, (size_t)2 * (n > 0 ? n : 1), Fill::kNone, fn, "the world"));
    if (n > 0) HIPC(hipMemcpyAsync(d_world, world_xy, sizeof(double) * 2 * n, hipMemcpyHostToDevice, P.stream));
    const ekf::SimParams p = to_sim(sp);
    if (!lidar) {
        ekf::launch_sim_unknown(p, B, n, T, jmax, d_world, P.ulog_twist, P.ulog_truth, P.ulog_count, P.ulog_meas, true, P.stream);
    } else {
        ekf::launch_sim_unknown(p, B, n, T, jmax, d_world, P.ulog_twist, P.ulog_truth, nullptr, nullptr, true, P.stream);
        const ekf::LidarParams lp = to_lidar(lidar);
        // scans are produced and consumed in chunks of whole steps (<= 256 MiB of ranges at a time)
        size_t steps_per_chunk = ((size_t)256 << 20) / (sizeof(double) * lp.n_beams * B);
        if (steps_per_chunk < 1) steps_per_chunk = 1;
        if (steps_per_chunk > (size_t)T) steps_per_chunk = T;
        EKFC(tmp.alloc(&d_ranges, steps_per_chunk * B * lp.n_beams, Fill::kNone, fn, "the scans"));
        EKFC(tmp.alloc(&d_radii, steps_per_chunk * B * jmax, Fill::kNone, fn, "the radii"));
        for (int t0 = 0; t0 < T; t0 += (int)steps_per_chunk) {
            const int tc = T - t0 < (int)steps_per_chunk ? T - t0 : (int)steps_per_chunk;
            const int S = tc * B;
            ekf::launch_sim_scans(p, lp, B, n, S, t0, d_world, P.ulog_truth + (size_t)t0 * B * 3, d_ranges, P.stream);
            ekf::launch_circles(d_ranges, S, lp.n_beams, jmax, P.ulog_meas + (size_t)t0 * B * jmax * 2, d_radii,
                                P.ulog_count + (size_t)t0 * B, nullptr, nullptr, P.stream);
        }
    }
    HIPC(hipGetLastError());
    P.ucount_host.assign(n_ct, 0);
    HIPC(hipMemcpyAsync(P.ucount_host.data(), P.ulog_count, sizeof(int) * n_ct, hipMemcpyDeviceToHost, P.stream));
    HIPC(hipStreamSynchronize(P.stream));
    // decisions start as "not run" (-2)
    {
        std::vector<int> fill(n_as, -2);
        HIPC(hipMemcpy(P.ulog_assoc, fill.data(), sizeof(int) * n_as, hipMemcpyHostToDevice));
    }
    P.uT = T;
    P.ujmax = jmax;
    P.truth_is_unknown_log = 1;
    return EKF_OK;
}

ekf_status ekf_batch_download_unknown_log(ekf_batch_handle hb, double* twist, int* count, double* meas_xy,
                                          double* true_pose) {
    if (!hb) return fail(EKF_ERR_INVALID, "null handle");
    Pool& P = hb->pool;
    if (P.uT <= 0) return fail(EKF_ERR_STATE, "no unknown-association log on the device");
    if (true_pose && !P.ulog_truth) return fail(EKF_ERR_STATE, "the uploaded log carries no simulated truth");
    EKFC(P.use());
    HIPC(hipStreamSynchronize(P.stream));
    const size_t B = P.pv.B, T = P.uT, J = P.ujmax;
    if (twist) HIPC(hipMemcpy(twist, P.ulog_twist, sizeof(double) * T * B * 2, hipMemcpyDeviceToHost));
    if (count) HIPC(hipMemcpy(count, P.ulog_count, sizeof(int) * T * B, hipMemcpyDeviceToHost));
    if (meas_xy && J) HIPC(hipMemcpy(meas_xy, P.ulog_meas, sizeof(double) * T * B * J * 2, hipMemcpyDeviceToHost));
    if (true_pose) HIPC(hipMemcpy(true_pose, P.ulog_truth, sizeof(double) * T * B * 3, hipMemcpyDeviceToHost));
    return EKF_OK;
}

ekf_status ekf_simulate_scans(int device, const ekf_sim_params* sp, const ekf_lidar_params* lidar, const double* world_xy,
                              int n, const double* poses, int S, int step, double* ranges_out) {
    if (!sp || !lidar || !lidar_ok(lidar) || n < 0 || (n > 0 && !world_xy) || S < 0 || (S > 0 && (!poses || !ranges_out)) ||
        step < 0)
        return fail(EKF_ERR_INVALID, "ekf_simulate_scans: bad argument (8 <= n_beams <= 1024)");
    if (S == 0) return EKF_OK;
    EKFC(select_device(&device, false));
    HIPC(hipSetDevice(device));
    ScopedMem tmp;
    double *d_world = nullptr, *d_poses = nullptr, *d_ranges = nullptr;
    EKFC(tmp.replace_group({target(&d_world, (size_t)2 * (n > 0 ? n : 1)), target(&d_poses, (size_t)3 * S),
                            target(&d_ranges, (size_t)S * lidar->n_beams)}, "ekf_simulate_scans", "the world, poses and scans"));
    if (n > 0) HIPC(hipMemcpy(d_world, world_xy, sizeof(double) * 2 * n, hipMemcpyHostToDevice));
    HIPC(hipMemcpy(d_poses, poses, sizeof(double) * 3 * S, hipMemcpyHostToDevice));
    // B = S, t0 = step: scan s draws the noise stream of filter first_filter_id + s at that step
    ekf::launch_sim_scans(to_sim(sp), to_lidar(lidar), S, n, S, step, d_world, d_poses, d_ranges, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(ranges_out, d_ranges, sizeof(double) * (size_t)S * lidar->n_beams, hipMemcpyDeviceToHost));
    return EKF_OK;
}

ekf_status ekf_normalize_angles(int device, const double* in, int count, double* out) {
    if (count < 0 || (count > 0 && (!in || !out))) return fail(EKF_ERR_INVALID, "ekf_normalize_angles: bad argument");
    if (count == 0) return EKF_OK;
    EKFC(select_device(&device, false));
    HIPC(hipSetDevice(device));
    ScopedMem tmp;
    double *d_in = nullptr, *d_out = nullptr;
    EKFC(tmp.replace_group({target(&d_in, (size_t)count), target(&d_out, (size_t)count)}, "ekf_normalize_angles", "the angles"));
    HIPC(hipMemcpy(d_in, in, sizeof(double) * count, hipMemcpyHostToDevice));
    ekf::launch_normalize_angles(d_in, count, d_out, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(out, d_out, sizeof(double) * count, hipMemcpyDeviceToHost));
    return EKF_OK;
}

ekf_status ekf_circle_fit_scans(int device, const double* ranges, int S, int n_beams, int max_out, double* centres,
                                double* radii, int* counts, double* all_clusters, int* n_clusters) {
    if (!ranges || !centres || !radii || !counts || S < 0 || n_beams < 1 || max_out < 1 ||
        n_beams > ekf::circles_max_beams())
        return fail(EKF_ERR_INVALID, "ekf_circle_fit_scans: bad argument (n_beams must be 1..1024)");
    if (S == 0) return EKF_OK;
    const char* fn = "ekf_circle_fit_scans";
    EKFC(select_device(&device, false));
    HIPC(hipSetDevice(device));
    const size_t nS = (size_t)S, n_c = nS * max_out * 2, n_rad = nS * max_out, n_all = nS * ekf::circles_max_clusters() * 4;
    ScopedMem tmp;
    double *d_r = nullptr, *d_c = nullptr, *d_rad = nullptr, *d_all = nullptr;
    int *d_cnt = nullptr, *d_nc = nullptr;
    EKFC(tmp.replace_group({target(&d_r, nS * n_beams), target(&d_c, n_c, Fill::kZero), target(&d_rad, n_rad, Fill::kZero),
                            target(&d_cnt, nS), target(&d_nc, nS)}, fn, "the scans and circles"));
    if (all_clusters) EKFC(tmp.alloc(&d_all, n_all, Fill::kZero, fn, "the clusters"));
    HIPC(hipMemcpy(d_r, ranges, sizeof(double) * nS * n_beams, hipMemcpyHostToDevice));
    ekf::launch_circles(d_r, S, n_beams, max_out, d_c, d_rad, d_cnt, d_all, d_nc, nullptr);
    HIPC(hipGetLastError());
    HIPC(hipMemcpy(centres, d_c, sizeof(double) * n_c, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(radii, d_rad, sizeof(double) * n_rad, hipMemcpyDeviceToHost));
    HIPC(hipMemcpy(counts, d_cnt, sizeof(int) * nS, hipMemcpyDeviceToHost));
    if (n_clusters) HIPC(hipMemcpy(n_clusters, d_nc, sizeof(int) * nS, hipMemcpyDeviceToHost));
    if (all_clusters) HIPC(hipMemcpy(all_clusters, d_all, sizeof(double) * n_all, hipMemcpyDeviceToHost));
    return EKF_OK;
}

}  // extern "C"
