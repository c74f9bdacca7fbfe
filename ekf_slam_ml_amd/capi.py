"""ctypes binding of libekfslam_hip.so (include/ekfslam.h) -- the only way Python reaches the filter.

There is no fallback: if the shared library is missing or no gfx950 device is visible, every
constructor raises.  The classes mirror the reference's call surface:

  EKF_SLAM      rigid2d::EKF_SLAM                      rigid2d/include/rigid2d/ekf_slam.hpp:19-57
  BatchEKF      B independent EKF_SLAM objects driven by a device-resident log (configs[4])
  DenseEKFSLAM  rigid2d::EKF_SLAM's three methods on one fp64 dense handle (DensePropagator64)
"""
from __future__ import annotations

import ctypes as C
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EKF_LIB_PATH", os.path.join(_HERE, "libekfslam_hip.so"))  # (override: A/B of two builds)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_bp = C.POINTER(C.c_uint8)
_fp = C.POINTER(C.c_float)

STATUS = {0: "EKF_OK", 1: "EKF_ERR_INVALID", 2: "EKF_ERR_NO_DEVICE", 3: "EKF_ERR_HIP", 4: "EKF_ERR_NOMEM",
          5: "EKF_ERR_STATE"}

# every symbol include/ekfslam.h declares (tests/test_host.py checks the .so exports them all)
SYMBOLS = [
    "ekf_last_error", "ekf_default_params", "ekf_leading_dimension", "ekf_device_count",
    "ekf_create", "ekf_destroy", "ekf_clone", "ekf_predict", "ekf_measure_known", "ekf_associate",
    "ekf_maha_scores", "ekf_get_pose", "ekf_get_landmarks", "ekf_dim", "ekf_get_state", "ekf_set_state",
    "ekf_get_cov", "ekf_set_cov", "ekf_get_init_flag", "ekf_set_init_flag", "ekf_sync", "ekf_device_bytes", "ekf_set_tuning", "ekf_set_active_set", "ekf_batch_set_active_set", "ekf_batch_get_touched",
    "ekf_batch_create", "ekf_batch_destroy", "ekf_batch_reset", "ekf_batch_device_bytes",
    "ekf_batch_upload_known_log", "ekf_batch_run_known", "ekf_batch_upload_unknown_log", "ekf_batch_run_unknown",
    "ekf_batch_get_known_counts", "ekf_batch_get_decisions", "ekf_batch_get_state", "ekf_batch_get_cov",
    "ekf_batch_get_poses", "ekf_batch_checksum", "ekf_batch_set_tuning",
    "ekf_set_update_mode", "ekf_batch_set_update_mode",
    "ekf_default_sim_params", "ekf_batch_simulate_known_log", "ekf_batch_download_log", "ekf_batch_mc_stats",
    "ekf_circle_fit_scans", "ekf_normalize_angles",
    "ekf_default_lidar_params", "ekf_batch_simulate_unknown_log", "ekf_batch_download_unknown_log", "ekf_simulate_scans",
    "ekf_dense_create", "ekf_dense_destroy", "ekf_dense_set", "ekf_dense_propagate", "ekf_dense_get_sigma",
    "ekf_dense_launch_info", "ekf_dense_tile_map",
    "ekf_dense64_create", "ekf_dense64_destroy", "ekf_dense64_set", "ekf_dense64_propagate", "ekf_dense64_get_sigma",
    "ekf_dense64_launch_info", "ekf_dense64_tile_map",
    "ekf_dense64_set_state", "ekf_dense64_get_state", "ekf_dense64_correct", "ekf_dense64_score", "ekf_dense64_propagate_block",
    "ekf_dense64_correct_sparse", "ekf_dense64_score_sparse",
    "ekf_dense64_correct_sparse_deferred", "ekf_dense64_flush", "ekf_dense64_pending",
    "ekf_dense64_correct_sparse_joseph", "ekf_dense64_joseph_launch_info",
    "ekf_dense64_score_landmarks", "ekf_dense64_associate_landmarks",
    "ekf_dense64_fit_scan", "ekf_dense64_associate_scan",
    "ekf_dense64_score_readings", "ekf_dense64_joint_operands", "ekf_dense64_associate_joint",
    "ekf_dense64_associate_scan_joint",
    "ekf_dense64_jcbb_launch_info", "ekf_dense64_jcbb_candidates", "ekf_dense64_jcbb_search", "ekf_dense64_associate_jcbb",
    "ekf_dense64_associate_scan_jcbb",
    "ekf_dense64_predict_landmarks", "ekf_dense64_measure_landmarks",
    "ekf_dense64_set_carry", "ekf_dense64_get_carry",
    "ekf_dense64_set_live", "ekf_dense64_get_live", "ekf_dense64_coupling",
    "ekf_dense64_region_begin", "ekf_dense64_region_end", "ekf_dense64_region_info", "ekf_dense64_region_launch_info",
    "ekf_dense64_get_padded",
    "ekf_dense64_pairs_launch_info", "ekf_dense64_score_landmark_pairs", "ekf_dense64_merge_landmarks",
    "ekf_dense64_remove_landmark",
    "ekf_dense64_evidence_launch_info", "ekf_dense64_scan_evidence", "ekf_dense64_evidence_update",
    "ekf_dense64_health_launch_info", "ekf_dense64_health", "ekf_dense64_symmetrize",
    "ekf_dense64_value_launch_info", "ekf_dense64_value_operands", "ekf_dense64_rank_landmarks",
    "ekf_dense64_factor_launch_info", "ekf_dense64_factor", "ekf_dense64_get_factor", "ekf_dense64_whiten",
    "ekf_dense64_solve_launch_info", "ekf_dense64_solve", "ekf_dense64_color",
    "ekf_dense64_frame_launch_info", "ekf_dense64_map_congruence", "ekf_dense64_reframe_landmarks",
    "ekf_dense64_join_launch_info", "ekf_dense64_join_congruence", "ekf_dense64_join_map",
    "ekf_dense64_extract_launch_info", "ekf_dense64_extract_map",
    "ekf_dense64_init_block", "ekf_dense64_swap_blocks", "ekf_dense64_get_sigma_block", "ekf_dense64_get_state_block", "ekf_dense64_set_state_block",
    "ekf_batch_rank2_variant", "ekf_batch_rank2_resident", "ekf_batch_rank2_packing", "ekf_batch_spec_counts",
    "ekf_batch_set_chain", "ekf_batch_chain_counts",
    "ekf_set_profiling", "ekf_get_profile", "ekf_batch_set_known_counts",
    "ekf_set_forms", "ekf_get_forms", "ekf_batch_set_forms", "ekf_batch_get_forms", "ekf_batch_form_counts",
    "ekf_phase_trace", "ekf_test_raise_device_error",
]

# ekf_form (include/ekfslam.h): launch structures the library may take where they apply; all exact forms are bit-identical
FORM_SMALL_MAP, FORM_CALL_FUSED, FORM_ACTIVE_PREFIX = 1 << 0, 1 << 2, 1 << 3   # (1 << 1: retired, ignored)
FORM_STEP_FUSED, FORM_STEP_SPLIT_PASS, FORM_DELAYED_PAIR, FORM_ROW_PACKING = 1 << 4, 1 << 5, 1 << 6, 1 << 7
FORM_STRIP_FLUSH, FORM_STRIP_FLUSH_ALWAYS = 1 << 8, 1 << 9
FORM_COLUMN_PANEL, FORM_COLUMN_PANEL_ONE_SLOT, FORM_STEP_SPECULATE, FORM_CURRENT_COLUMNS = 1 << 10, 1 << 11, 1 << 12, 1 << 13
FORM_TILE_QUEUE, FORM_STEP_CHAIN = 1 << 14, 1 << 15
FORMS_DEFAULT = (((1 << 9) - 1) | FORM_COLUMN_PANEL | FORM_STEP_SPECULATE | FORM_CURRENT_COLUMNS | FORM_TILE_QUEUE
                 | FORM_STEP_CHAIN)
CHAIN_POLICY_EXPLICIT = 16   # set_chain(policy=CHAIN_POLICY_EXPLICIT | bits): the four bits as given (0 = automatic)


class EkfError(RuntimeError):
    def __init__(self, status, text):
        super().__init__(f"{STATUS.get(status, status)}: {text}")
        self.status = status


class Params(C.Structure):
    """ekf_params (include/ekfslam.h); defaults are the reference's hard-coded constants."""
    _fields_ = [("sigma0_landmark", C.c_double), ("q_pose", C.c_double), ("r_meas", C.c_double),
                ("gate_new", C.c_double), ("gate_update", C.c_double), ("straight_eps", C.c_double)]


class HealthReport(C.Structure):
    """ekf_dense64_health_report (include/ekfslam.h)"""
    _fields_ = [("n_nonfinite", C.c_longlong), ("n_asym", C.c_longlong), ("n_diag_bad", C.c_longlong),
                ("n_minor", C.c_longlong), ("max_asym", C.c_double), ("min_diag", C.c_double),
                ("asym_i", C.c_int), ("asym_j", C.c_int), ("min_diag_i", C.c_int), ("reserved", C.c_int)]


class ValueBest(C.Structure):
    """ekf_dense64_value_best (include/ekfslam.h)"""
    _fields_ = [("i_trace", C.c_int), ("i_pose", C.c_int), ("i_det", C.c_int), ("reserved", C.c_int),
                ("v_trace", C.c_double), ("v_pose", C.c_double), ("v_det", C.c_double)]


class EvidenceReport(C.Structure):
    """ekf_dense64_evidence_report (include/ekfslam.h)"""
    _fields_ = [("n_candidates", C.c_int), ("n_on_tube", C.c_int), ("n_unexplained", C.c_int), ("n_invalid", C.c_int)]


class ScanEvidence:
    """What scan_evidence() returns: per landmark n_expected, n_agree, n_through, n_short (count,) int32 and tol (count,);
    per beam expected (n_beams,), hit (n_beams,) int32 (the landmark index, -1 for the wall or range_max) and cls
    (n_beams,) uint8 (0 wall / range_max, 1 agree, 2 through, 3 short, 4 invalid); report = {n_candidates, n_on_tube,
    n_unexplained, n_invalid}; first_lm; ms."""

    def __init__(self, first_lm, n_expected, n_agree, n_through, n_short, tol, expected, hit, cls, report, ms):
        self.first_lm, self.n_expected, self.n_agree, self.n_through, self.n_short = first_lm, n_expected, n_agree, n_through, n_short
        self.tol, self.expected, self.hit, self.cls, self.ms = tol, expected, hit, cls, ms
        self.report = {name: getattr(report, name) for name, _ in EvidenceReport._fields_}


def evidence_update(logodds, n_expected, n_agree, n_through, min_beams=3, w_hit=0.4, w_miss=0.85, l_min=-4.0, l_max=4.0):
    """ekf_dense64_evidence_update (no handle, no device): per landmark with n_expected >= min_beams a hit (2 n_agree >=
    n_expected: l += w_hit) or a miss (2 n_through > n_expected: l -= w_miss), then the clamp to [l_min, l_max].  logodds
    (count,) float64 is updated IN PLACE; returns verdict (count,) int32: +1 hit, -1 miss, 0 neither."""
    if not (isinstance(logodds, np.ndarray) and logodds.dtype == np.float64 and logodds.ndim == 1 and logodds.flags.c_contiguous):
        raise ValueError("logodds must be a contiguous float64 array of one dimension (it is updated in place)")
    n = logodds.shape[0]
    cnt = [np.ascontiguousarray(a, dtype=np.int32) for a in (n_expected, n_agree, n_through)]
    if any(a.shape != (n,) for a in cnt):
        raise ValueError("the counters must hold one entry per log-odds value")
    verdict = np.zeros(n, dtype=np.int32)
    if n == 0:
        return verdict
    _check(load().ekf_dense64_evidence_update(n, cnt[0].ctypes.data_as(_ip), cnt[1].ctypes.data_as(_ip),
                                              cnt[2].ctypes.data_as(_ip), int(min_beams), float(w_hit), float(w_miss),
                                              float(l_min), float(l_max), _d(logodds), verdict.ctypes.data_as(_ip)))
    return verdict


class ObservationValue:
    """What value_operands() / rank_landmarks() return: per landmark dtrace, dtrace_pose, detS, S (count, 2, 2), flags,
    in_view, Hc (count, 2, 5); info_gain = 0.5 * log(detS / det R), formed on the host; best = {i_trace, i_pose, i_det,
    v_trace, v_pose, v_det} (index -1: nothing eligible); first_lm; ms."""

    def __init__(self, first_lm, dtrace, dtrace_pose, detS, S, flags, in_view, Hc, R, best, ms):
        self.first_lm, self.dtrace, self.dtrace_pose, self.detS, self.S, self.flags = first_lm, dtrace, dtrace_pose, detS, S, flags
        self.in_view, self.Hc, self.R, self.ms = in_view, Hc, R, ms
        with np.errstate(all="ignore"):
            self.info_gain = 0.5 * np.log(detS / (R[0, 0] * R[1, 1] - R[0, 1] * R[1, 0]))
        self.best = {name: getattr(best, name) for name, _ in ValueBest._fields_ if name != "reserved"}

    def order(self, by="trace"):
        """the indices j in [0, count) of the eligible landmarks (flag 0, in view, value not a NaN), best first; a stable
        sort, so the lower index comes first among equal values"""
        if by not in ("trace", "pose", "info"):
            raise ValueError('by: "trace", "pose" or "info"')
        v = {"trace": self.dtrace, "pose": self.dtrace_pose, "info": self.info_gain}[by]
        ok = np.flatnonzero((self.flags == 0) & (self.in_view != 0) & ~np.isnan(v))
        return ok[np.argsort(-v[ok], kind="stable")]


class JcbbReport(C.Structure):
    """ekf_dense64_jcbb_report (include/ekfslam.h)"""
    _fields_ = [("n_cand", C.c_int), ("n_pairs", C.c_int), ("n_new", C.c_int), ("n_drop", C.c_int), ("exhausted", C.c_int),
                ("nodes", C.c_longlong), ("d2", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class RegionReport(C.Structure):
    """ekf_dense64_region_report (include/ekfslam.h)"""
    _fields_ = [("Na", C.c_int), ("Nb", C.c_int), ("corrections", C.c_longlong), ("row_maps", C.c_longlong),
                ("group_bytes", C.c_longlong)]


class FactorReport(C.Structure):
    """ekf_dense64_factor_report (include/ekfslam.h)"""
    _fields_ = [("ok", C.c_int), ("fail_index", C.c_int), ("min_pivot_i", C.c_int), ("Na", C.c_int),
                ("fail_pivot", C.c_double), ("min_pivot", C.c_double), ("max_pivot", C.c_double), ("logdet", C.c_double)]


class KnownLogC(C.Structure):
    _fields_ = [("T", C.c_int), ("vmax", C.c_int), ("twist", _dp), ("lm_idx", _ip), ("z_xy", _dp), ("init_xy", _dp)]


class UnknownLogC(C.Structure):
    _fields_ = [("T", C.c_int), ("jmax", C.c_int), ("twist", _dp), ("count", _ip), ("meas_xy", _dp)]


class SimParams(C.Structure):
    """ekf_sim_params (include/ekfslam.h): noise model of the reference's simulator."""
    _fields_ = [("seed", C.c_ulonglong), ("first_filter_id", C.c_longlong), ("v_cmd", C.c_double), ("w_cmd", C.c_double),
                ("vx_std", C.c_double), ("the_std", C.c_double), ("slip_min", C.c_double), ("slip_max", C.c_double),
                ("sensor_std", C.c_double), ("max_visible_dis", C.c_double), ("wheel_base", C.c_double),
                ("wheel_radius", C.c_double), ("ticks_per_step", C.c_int)]


class LidarParams(C.Structure):
    """ekf_lidar_params (include/ekfslam.h): the simulator's 2-D lidar."""
    _fields_ = [("n_beams", C.c_int), ("range_std", C.c_double), ("range_max", C.c_double),
                ("border_width", C.c_double), ("tube_radius", C.c_double), ("model", C.c_int), ("range_min", C.c_double)]


def default_lidar(**kw):
    lp = LidarParams()
    load().ekf_default_lidar_params(C.byref(lp))
    for k, v in kw.items():
        setattr(lp, k, v)
    return lp


class RunStats(C.Structure):
    _fields_ = [("elapsed_ms", C.c_double), ("rank2_ms", C.c_double), ("rank2_launches", C.c_longlong),
                ("corrections", C.c_longlong), ("filter_steps", C.c_longlong),
                ("rank2_bytes_per_launch", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


_lib = None


def load():
    """Load libekfslam_hip.so; raises (never falls back) when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch bundles its own libamdhip64.so.7; if torch will be used in this process it must be loaded
    # first so that both share ONE HIP runtime (the dynamic loader dedups by SONAME).
    lib = C.CDLL(LIB_PATH)
    h = C.c_void_p
    lib.ekf_last_error.restype = C.c_char_p
    lib.ekf_default_params.argtypes = [C.POINTER(Params)]
    lib.ekf_leading_dimension.argtypes = [C.c_int]
    lib.ekf_leading_dimension.restype = C.c_int
    lib.ekf_device_count.restype = C.c_int
    lib.ekf_default_sim_params.argtypes = [C.POINTER(SimParams)]
    lib.ekf_default_lidar_params.argtypes = [C.POINTER(LidarParams)]
    lib.ekf_default_lidar_params.restype = None
    sig = {
        "ekf_create": [C.c_int, C.POINTER(Params), C.c_int, C.POINTER(h)],
        "ekf_destroy": [h],
        "ekf_clone": [h, C.POINTER(h)],
        "ekf_predict": [h, C.c_double, C.c_double],
        "ekf_measure_known": [h, _dp, _bp],
        "ekf_associate": [h, _dp, C.c_int, _bp, _ip],
        "ekf_maha_scores": [h, C.c_double, C.c_double, C.c_int, _dp],
        "ekf_get_pose": [h, _dp],
        "ekf_get_landmarks": [h, _dp],
        "ekf_dim": [h, _ip, _ip],
        "ekf_get_state": [h, _dp],
        "ekf_set_state": [h, _dp],
        "ekf_get_cov": [h, _dp],
        "ekf_set_cov": [h, _dp],
        "ekf_get_init_flag": [h, _ip],
        "ekf_set_init_flag": [h, C.c_int],
        "ekf_sync": [h],
        "ekf_device_bytes": [h, C.POINTER(C.c_size_t)],
        "ekf_set_active_set": [h, C.c_int],
        "ekf_batch_set_active_set": [h, C.c_int],
        "ekf_batch_get_touched": [h, _ip],
        "ekf_batch_upload_unknown_log": [h, C.POINTER(UnknownLogC)],
        "ekf_batch_run_unknown": [h, C.c_int, C.c_int, C.c_int, C.POINTER(RunStats)],
        "ekf_batch_get_known_counts": [h, _ip],
        "ekf_batch_get_decisions": [h, _ip],
        "ekf_set_tuning": [h, C.c_int, C.c_int, C.c_int],
        "ekf_batch_create": [C.c_int, C.c_int, C.POINTER(Params), C.c_int, C.POINTER(h)],
        "ekf_batch_destroy": [h],
        "ekf_batch_reset": [h],
        "ekf_batch_device_bytes": [h, C.POINTER(C.c_size_t)],
        "ekf_batch_upload_known_log": [h, C.POINTER(KnownLogC)],
        "ekf_batch_run_known": [h, C.c_int, C.c_int, C.c_int, C.POINTER(RunStats)],
        "ekf_batch_get_state": [h, C.c_int, _dp],
        "ekf_batch_get_cov": [h, C.c_int, _dp],
        "ekf_batch_get_poses": [h, _dp],
        "ekf_batch_checksum": [h, _dp],
        "ekf_batch_set_tuning": [h, C.c_int, C.c_int, C.c_int],
        "ekf_set_update_mode": [h, C.c_int, C.c_int],
        "ekf_batch_set_update_mode": [h, C.c_int, C.c_int],
        "ekf_batch_simulate_known_log": [h, C.POINTER(SimParams), _dp, C.c_int, C.c_int],
        "ekf_batch_download_log": [h, _dp, _ip, _dp, _dp, _dp],
        "ekf_batch_mc_stats": [h, C.c_int, _dp],
        "ekf_batch_simulate_unknown_log": [h, C.POINTER(SimParams), C.POINTER(LidarParams), _dp, C.c_int, C.c_int],
        "ekf_batch_download_unknown_log": [h, _dp, _ip, _dp, _dp],
        "ekf_simulate_scans": [C.c_int, C.POINTER(SimParams), C.POINTER(LidarParams), _dp, C.c_int, _dp, C.c_int,
                               C.c_int, _dp],
        "ekf_normalize_angles": [C.c_int, _dp, C.c_int, _dp],
        "ekf_circle_fit_scans": [C.c_int, _dp, C.c_int, C.c_int, C.c_int, _dp, _dp, _ip, _dp, _ip],
        "ekf_dense_create": [C.c_int, C.c_int, C.POINTER(h)],
        "ekf_dense_destroy": [h],
        "ekf_dense_set": [h, _fp, _fp, _fp],
        "ekf_dense_propagate": [h, C.c_int, _dp],
        "ekf_dense_get_sigma": [h, _fp],
        "ekf_dense_launch_info": [h, _ip, _ip, _ip, _ip],
        "ekf_dense_tile_map": [h, _bp],
        "ekf_dense64_create": [C.c_int, C.c_int, C.POINTER(h)],
        "ekf_dense64_destroy": [h],
        "ekf_dense64_set": [h, _dp, _dp, _dp],
        "ekf_dense64_propagate": [h, C.c_int, _dp],
        "ekf_dense64_get_sigma": [h, _dp],
        "ekf_dense64_launch_info": [h, _ip, _ip, _ip, _ip],
        "ekf_dense64_tile_map": [h, _bp],
        "ekf_dense64_set_state": [h, _dp],
        "ekf_dense64_get_state": [h, _dp],
        "ekf_dense64_correct": [h, C.c_int, _dp, _dp, _dp, _dp, _dp],
        "ekf_dense64_score": [h, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp, _ip, _dp],
        "ekf_dense64_propagate_block": [h, C.c_int, C.c_int, _dp, _dp, _dp, _dp],
        "ekf_dense64_correct_sparse": [h, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp],
        "ekf_dense64_score_sparse": [h, C.c_int, C.c_int, C.c_int, _ip, _dp, _dp, C.c_int, _dp, _dp, _dp, _ip, _dp],
        "ekf_dense64_correct_sparse_deferred": [h, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp],
        "ekf_dense64_correct_sparse_joseph": [h, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.POINTER(C.c_longlong),
                                              _dp],
        "ekf_dense64_joseph_launch_info": [h, _ip, _ip, _ip],
        "ekf_dense64_flush": [h, _dp],
        "ekf_dense64_pending": [h, _ip],
        "ekf_dense64_score_landmarks": [h, C.POINTER(Params), C.c_double, C.c_double, C.c_int, C.c_int, _dp, _dp, _ip, _ip,
                                        _dp, _dp, _dp],
        "ekf_dense64_associate_landmarks": [h, C.POINTER(Params), C.c_int, _dp, C.c_int, _ip, C.c_uint, _ip, _dp, _dp],
        "ekf_dense64_fit_scan": [h, _dp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _ip, _dp],
        "ekf_dense64_associate_scan": [h, C.POINTER(Params), _dp, C.c_int, C.c_int, C.c_int, _ip, C.c_uint, _ip, _dp, _ip,
                                       _dp, _dp],
        "ekf_dense64_score_readings": [h, C.POINTER(Params), C.c_int, _dp, C.c_int, C.c_int, _dp, _ip, _dp],
        "ekf_dense64_joint_operands": [h, C.POINTER(Params), C.c_int, _ip, _dp, _ip, _dp, _dp, _dp],
        "ekf_dense64_associate_joint": [h, C.POINTER(Params), C.c_int, _dp, C.c_int, _ip, C.c_uint, _ip, _dp, _ip, _dp],
        "ekf_dense64_associate_scan_joint": [h, C.POINTER(Params), _dp, C.c_int, C.c_int, C.c_int, _ip, C.c_uint, _ip, _dp,
                                             _ip, _dp, _dp],
        "ekf_dense64_jcbb_launch_info": [h, _ip, _ip],
        "ekf_dense64_jcbb_candidates": [h, C.POINTER(Params), C.c_int, _dp, C.c_int, C.c_double, C.c_int, _ip, _ip, _dp, _dp,
                                        _ip, _ip, _dp, _dp, _dp],
        "ekf_dense64_jcbb_search": [C.c_int, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, C.c_longlong, _ip, C.POINTER(JcbbReport)],
        "ekf_dense64_associate_jcbb": [h, C.POINTER(Params), C.c_int, _dp, C.c_int, _ip, C.c_double, _dp, C.c_longlong,
                                       C.c_uint, _ip, _dp, C.POINTER(JcbbReport), _ip, _dp],
        "ekf_dense64_associate_scan_jcbb": [h, C.POINTER(Params), _dp, C.c_int, C.c_int, C.c_int, _ip, C.c_double, _dp,
                                            C.c_longlong, C.c_uint, _ip, _dp, _ip, _dp, C.POINTER(JcbbReport), _dp],
        "ekf_dense64_predict_landmarks": [h, C.POINTER(Params), C.c_double, C.c_double, _dp, _dp, _dp],
        "ekf_dense64_measure_landmarks": [h, C.POINTER(Params), C.c_int, _dp, _bp, _ip, C.c_uint, _ip, _dp, _dp, _dp],
        "ekf_dense64_set_carry": [h, C.c_int],
        "ekf_dense64_get_carry": [h, _ip],
        "ekf_dense64_set_live": [h, C.c_int],
        "ekf_dense64_get_live": [h, _ip],
        "ekf_dense64_coupling": [h, C.c_int, C.POINTER(C.c_longlong), _dp, _dp],
        "ekf_dense64_get_padded": [h, _dp, _dp],
        "ekf_dense64_region_begin": [h, C.c_int, _dp],
        "ekf_dense64_region_end": [h, C.POINTER(RegionReport), _dp],
        "ekf_dense64_region_info": [h, _ip, _ip] + [C.POINTER(C.c_longlong)] * 3,
        "ekf_dense64_region_launch_info": [h, C.c_int] + [_ip] * 7 + [C.POINTER(C.c_longlong)],
        "ekf_dense64_pairs_launch_info": [h, _ip, _ip],
        "ekf_dense64_score_landmark_pairs": [h, C.c_int, C.c_double, C.c_double, _ip, _dp, C.POINTER(C.c_longlong),
                                             C.POINTER(C.c_longlong), _dp],
        "ekf_dense64_merge_landmarks": [h, C.POINTER(Params), C.c_int, C.c_int, C.c_double, _ip, C.c_int, _ip, _dp, _dp],
        "ekf_dense64_remove_landmark": [h, C.POINTER(Params), C.c_int, _ip, C.c_uint, _ip, _dp],
        "ekf_dense64_evidence_launch_info": [h, _ip, _ip, _ip],
        "ekf_dense64_scan_evidence": [h, C.POINTER(Params), C.POINTER(LidarParams), _dp, C.c_int, C.c_int, C.c_double,
                                      C.c_double, _ip, _ip, _ip, _ip, _dp, _dp, _ip, _bp, C.POINTER(EvidenceReport), _dp],
        "ekf_dense64_evidence_update": [C.c_int, _ip, _ip, _ip, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                        _dp, _ip],
        "ekf_dense64_health_launch_info": [h, _ip, _ip],
        "ekf_dense64_health": [h, C.POINTER(HealthReport), _dp],
        "ekf_dense64_symmetrize": [h, C.POINTER(C.c_longlong), _dp, _dp],
        "ekf_dense64_value_launch_info": [h, _ip, _ip, _ip],
        "ekf_dense64_value_operands": [h, C.c_int, C.c_int, _dp, _dp, _bp, _dp, _dp, _dp, _dp, _ip, C.POINTER(ValueBest), _dp],
        "ekf_dense64_rank_landmarks": [h, C.POINTER(Params), C.c_int, C.c_int, C.c_double, _dp, _dp, _dp, _dp, _ip,
                                       C.POINTER(ValueBest), _bp, _dp, _dp],
        "ekf_dense64_factor_launch_info": [h, _ip, _ip],
        "ekf_dense64_factor": [h, C.POINTER(FactorReport), _dp],
        "ekf_dense64_get_factor": [h, _dp],
        "ekf_dense64_whiten": [h, C.c_int, _dp, _dp, _dp, _dp],
        "ekf_dense64_solve_launch_info": [h, _ip, _ip, _ip],
        "ekf_dense64_solve": [h, C.c_int, _dp, _dp, _dp, _dp, _dp],
        "ekf_dense64_color": [h, C.c_int, _dp, C.c_int, _dp, _dp],
        "ekf_dense64_frame_launch_info": [h, _ip, _ip, _ip],
        "ekf_dense64_map_congruence": [h, _dp, _dp, _dp],
        "ekf_dense64_reframe_landmarks": [h, C.c_int, C.c_double, C.c_double, C.c_double, _dp, _dp],
        "ekf_dense64_join_launch_info": [h, _ip, _ip, _ip],
        "ekf_dense64_join_congruence": [h, h, _dp, _dp, _dp],
        "ekf_dense64_join_map": [h, h, _dp, _dp],
        "ekf_dense64_extract_launch_info": [h, _ip, _ip, _ip],
        "ekf_dense64_extract_map": [h, h, C.c_int, _ip, _dp],
        "ekf_dense64_init_block": [h, C.c_int, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp],
        "ekf_dense64_swap_blocks": [h, C.c_int, C.c_int, C.c_int, _dp],
        "ekf_dense64_get_sigma_block": [h, C.c_int, _ip, C.c_int, _ip, _dp],
        "ekf_dense64_get_state_block": [h, C.c_int, C.c_int, _dp],
        "ekf_dense64_set_state_block": [h, C.c_int, C.c_int, _dp],
        "ekf_batch_rank2_variant": [h, _ip, _ip, _ip, _ip],
        "ekf_batch_rank2_resident": [h, _ip],
        "ekf_batch_rank2_packing": [h, _ip],
        "ekf_batch_spec_counts": [h, C.POINTER(C.c_longlong)],
        "ekf_batch_set_chain": [h, C.c_int, C.c_int],
        "ekf_batch_chain_counts": [h, C.POINTER(C.c_longlong)],
        "ekf_batch_set_known_counts": [h, _ip],
        "ekf_set_profiling": [h, C.c_int],
        "ekf_set_forms": [h, C.c_uint],
        "ekf_get_forms": [h, C.POINTER(C.c_uint)],
        "ekf_batch_set_forms": [h, C.c_uint],
        "ekf_batch_get_forms": [h, C.POINTER(C.c_uint)],
        "ekf_batch_form_counts": [h, C.POINTER(C.c_longlong)],
        "ekf_phase_trace": [h, C.c_int, C.POINTER(C.c_longlong)],
        "ekf_test_raise_device_error": [h],
        "ekf_get_profile": [h, _dp, C.POINTER(C.c_longlong)],
    }
    for name, argtypes in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    _lib = lib
    return lib


def _check(st):
    if st != 0:
        raise EkfError(st, load().ekf_last_error().decode(errors="replace"))


def device_count():
    return load().ekf_device_count()


def leading_dimension(n):
    """doubles between two rows of a filter's covariance for a map of n landmarks (ekf_leading_dimension; needs no device)"""
    return load().ekf_leading_dimension(int(n))


def default_params():
    p = Params()
    load().ekf_default_params(C.byref(p))
    return p


def _d(a):
    return a.ctypes.data_as(_dp)


class EKF_SLAM:
    """rigid2d::EKF_SLAM over the C ABI: same method names, argument meaning and in/out behaviour
    as rigid2d/include/rigid2d/ekf_slam.hpp:19-57 (arma::mat -> float64 array,
    std::vector<bool> -> uint8 array, Twist2D -> (angular, linearX), Vector2D -> (x, y) rows)."""

    def __init__(self, n_measurements, params=None, device=-1, _handle=None):
        self._lib = load()
        self.n = int(n_measurements)
        self.N = 3 + 2 * self.n
        if _handle is not None:
            self._h = _handle
            return
        h = C.c_void_p()
        _check(self._lib.ekf_create(self.n, C.byref(params) if params is not None else None, device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ekf_destroy(self._h)
            self._h = None

    __del__ = close

    def clone(self):
        """Copy construction / assignment (slam_agent = EKF_SLAM(n), nuslam/src/slam.cpp:428)."""
        h = C.c_void_p()
        _check(self._lib.ekf_clone(self._h, C.byref(h)))
        return EKF_SLAM(self.n, _handle=h)

    def prediction(self, twist):
        """twist = (angular, linearX[, linearY]); linearY is ignored like ekf_slam.cpp:70."""
        _check(self._lib.ekf_predict(self._h, float(twist[0]), float(twist[1])))

    def measurement(self, sensor_reading, visible_list, known_list=None):
        s = np.ascontiguousarray(sensor_reading, dtype=np.float64).reshape(-1)
        v = np.ascontiguousarray(visible_list, dtype=np.uint8).reshape(-1)
        if s.size != 2 * self.n or v.size != self.n:
            raise ValueError("sensor_reading must hold 2n values and visible_list n")
        _check(self._lib.ekf_measure_known(self._h, _d(s), v.ctypes.data_as(_bp)))

    def data_association(self, measures, known_list):
        """known_list: uint8 ndarray of n entries, updated IN PLACE (ekf_slam.cpp:323).
        Returns the landmark each measurement corrected (-1 = dropped)."""
        m = np.ascontiguousarray(measures, dtype=np.float64).reshape(-1, 2)
        if not (isinstance(known_list, np.ndarray) and known_list.dtype == np.uint8
                and known_list.size == self.n and known_list.flags.c_contiguous):
            raise ValueError("known_list must be a contiguous uint8 array of n entries (it is in/out)")
        assoc = np.full(len(m), -1, dtype=np.int32)
        _check(self._lib.ekf_associate(self._h, _d(m), len(m), known_list.ctypes.data_as(_bp),
                                       assoc.ctypes.data_as(_ip)))
        return assoc

    def maha_scores(self, measure, M):
        out = np.empty(int(M))
        _check(self._lib.ekf_maha_scores(self._h, float(measure[0]), float(measure[1]), int(M), _d(out)))
        return out

    def _pose(self):
        out = np.empty(3)
        _check(self._lib.ekf_get_pose(self._h, _d(out)))
        return out

    def getStateX(self):
        return float(self._pose()[1])

    def getStateY(self):
        return float(self._pose()[2])

    def getStateTheta(self):
        return float(self._pose()[0])

    def getStateLandmark(self):
        out = np.empty(2 * self.n)
        _check(self._lib.ekf_get_landmarks(self._h, _d(out)))
        return out

    @property
    def state(self):
        out = np.empty(self.N)
        _check(self._lib.ekf_get_state(self._h, _d(out)))
        return out

    @state.setter
    def state(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        if v.size != self.N:
            raise ValueError("state must hold N = 3 + 2n values")
        _check(self._lib.ekf_set_state(self._h, _d(v)))

    @property
    def cov(self):
        out = np.empty((self.N, self.N))
        _check(self._lib.ekf_get_cov(self._h, _d(out)))
        return out

    @cov.setter
    def cov(self, v):
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (self.N, self.N):
            raise ValueError("cov must be N x N")
        _check(self._lib.ekf_set_cov(self._h, _d(v)))

    @property
    def landmark_init_flag(self):
        f = C.c_int()
        _check(self._lib.ekf_get_init_flag(self._h, C.byref(f)))
        return bool(f.value)

    @landmark_init_flag.setter
    def landmark_init_flag(self, f):
        _check(self._lib.ekf_set_init_flag(self._h, int(bool(f))))

    def sync(self):
        _check(self._lib.ekf_sync(self._h))

    def device_bytes(self):
        b = C.c_size_t()
        _check(self._lib.ekf_device_bytes(self._h, C.byref(b)))
        return b.value

    def set_active_set(self, enable=True):
        """Stream only the rows of the touched set in the eager correction (exact; opt-in)."""
        _check(self._lib.ekf_set_active_set(self._h, int(bool(enable))))

    @property
    def forms(self):
        f = C.c_uint()
        _check(self._lib.ekf_get_forms(self._h, C.byref(f)))
        return f.value

    def set_forms(self, forms=FORMS_DEFAULT):
        """which launch structures may be taken (FORM_* bits; test / measurement hook).  The forms a single filter takes are
        exact (bit-identical results); in delayed mode, what moves a flush moves the results at rounding level, inside the
        1e-9 contract -- BatchEKF.set_forms lists which forms are bit-identical and which agree to rounding"""
        _check(self._lib.ekf_set_forms(self._h, int(forms)))

    def _form(self, bit, enable):
        self.set_forms(self.forms | bit if enable else self.forms & ~bit)

    def set_small_map_path(self, enable=True):
        self._form(FORM_SMALL_MAP, enable)

    def set_active_prefix(self, enable=True):
        self._form(FORM_ACTIVE_PREFIX, enable)

    def set_call_fused(self, enable=True):
        """measurement() as two launches per call (factor panels + one pass over Sigma); default on, bit-identical"""
        self._form(FORM_CALL_FUSED, enable)

    def set_tuning(self, rows_per_block=0, nontemporal=-1, group_rows=0):
        _check(self._lib.ekf_set_tuning(self._h, rows_per_block, nontemporal, group_rows))

    def phase_trace(self, enable=True, fetch=False):
        """shader-clock stamps of the last two-launch measurement() call: array [2, 64] (row 0 the control wave, row 1
        the first slice wave of workgroup 0), or None"""
        out = np.zeros((2, 64), dtype=np.int64)
        _check(self._lib.ekf_phase_trace(self._h, int(bool(enable)),
                                         out.ctypes.data_as(C.POINTER(C.c_longlong)) if fetch else None))
        return out if fetch else None

    def set_profiling(self, enable=True):
        """HIP-event timing of every covariance-streaming (class 0) and scoring (class 1) launch; resets the sums"""
        _check(self._lib.ekf_set_profiling(self._h, int(bool(enable))))

    def profile(self):
        """{stream_ms, stream_launches, score_ms, score_launches} since set_profiling(True)"""
        ms = (C.c_double * 2)()
        ln = (C.c_longlong * 2)()
        _check(self._lib.ekf_get_profile(self._h, ms, ln))
        return {"stream_ms": ms[0], "stream_launches": ln[0], "score_ms": ms[1], "score_launches": ln[1]}

    def set_update_mode(self, max_pending_corrections=0, symmetric_gather=False):
        """0 = eager covariance stream per correction; k > 0 = delayed rank-2k update (flush every k); symmetric_gather:
        the opt-in symmetric option (Sigma H^T taken as (H Sigma)^T, mirrored flush) -- see ekf_set_update_mode"""
        _check(self._lib.ekf_set_update_mode(self._h, int(max_pending_corrections), int(symmetric_gather)))


class BatchEKF:
    """B independent filters on one GPU, replaying a device-resident known-association log."""

    def __init__(self, B, n, params=None, device=-1):
        self._lib = load()
        self.B, self.n, self.N = int(B), int(n), 3 + 2 * int(n)
        h = C.c_void_p()
        _check(self._lib.ekf_batch_create(self.B, self.n, C.byref(params) if params is not None else None,
                                          device, C.byref(h)))
        self._h = h
        self.T = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ekf_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def reset(self):
        _check(self._lib.ekf_batch_reset(self._h))

    def device_bytes(self):
        b = C.c_size_t()
        _check(self._lib.ekf_batch_device_bytes(self._h, C.byref(b)))
        return b.value

    def upload_known_log(self, twist, lm_idx, z_xy, init_xy):
        tw = np.ascontiguousarray(twist, dtype=np.float64)
        li = np.ascontiguousarray(lm_idx, dtype=np.int32)
        zz = np.ascontiguousarray(z_xy, dtype=np.float64)
        ii = np.ascontiguousarray(init_xy, dtype=np.float64)
        T, B = tw.shape[0], tw.shape[1]
        if B != self.B or tw.shape != (T, B, 2) or li.shape[:2] != (T, B) or zz.shape != li.shape + (2,) \
                or ii.shape != (B, 2 * self.n):
            raise ValueError("log arrays must be twist[T,B,2], lm_idx[T,B,vmax], z_xy[T,B,vmax,2], init_xy[B,2n]")
        log = KnownLogC(T, li.shape[2], _d(tw), li.ctypes.data_as(_ip), _d(zz), _d(ii))
        _check(self._lib.ekf_batch_upload_known_log(self._h, C.byref(log)))
        self.T, self._vmax = T, li.shape[2]

    def _sim_params(self, cfg):
        sp = SimParams()
        self._lib.ekf_default_sim_params(C.byref(sp))
        sp.seed, sp.first_filter_id = int(cfg.seed), int(cfg.first_filter_id)
        sp.v_cmd, sp.w_cmd, sp.vx_std, sp.the_std = cfg.v_cmd, cfg.w_cmd, cfg.vx_std, cfg.the_std
        sp.slip_min, sp.slip_max, sp.sensor_std, sp.max_visible_dis = cfg.slip_min, cfg.slip_max, cfg.sensor_std, cfg.max_visible_dis
        sp.ticks_per_step = cfg.ticks_per_step
        return sp

    def simulate_unknown_log(self, cfg, world, steps=None, jmax=None, lidar=None):
        """Unknown-association inputs generated ON THE DEVICE: the fake sensor's shuffled readings (lidar=None;
        host twin synth.make_unknown_log) or simulated laser scans pushed through the batched circle fitting
        (lidar = LidarParams; host twins synth.make_scans + the circle checker)."""
        w = np.ascontiguousarray(world, dtype=np.float64)
        if w.shape != (self.n, 2):
            raise ValueError("world must be [n, 2]")
        T = int(cfg.steps if steps is None else steps)
        J = int(cfg.vmax if jmax is None else jmax)
        sp = self._sim_params(cfg)
        _check(self._lib.ekf_batch_simulate_unknown_log(self._h, C.byref(sp), C.byref(lidar) if lidar is not None else None,
                                                        _d(w), T, J))
        self.uT, self._jmax = T, J

    def download_unknown_log(self, want_truth=True):
        T, B, J = self.uT, self.B, self._jmax
        tw, ct, me = np.empty((T, B, 2)), np.empty((T, B), dtype=np.int32), np.empty((T, B, J, 2))
        tp = np.empty((T, B, 3)) if want_truth else None
        _check(self._lib.ekf_batch_download_unknown_log(self._h, _d(tw), ct.ctypes.data_as(_ip), _d(me),
                                                        _d(tp) if want_truth else None))
        return tw, ct, me, tp

    def simulate_known_log(self, cfg, world, steps=None, vmax=None):
        """Generate the log ON THE DEVICE from a synth.SimConfig (same noise model and random-number
        addressing as synth.make_known_log, which stays the host-side twin for the tests)."""
        sp = SimParams()
        self._lib.ekf_default_sim_params(C.byref(sp))
        sp.seed, sp.first_filter_id = int(cfg.seed), int(cfg.first_filter_id)
        sp.v_cmd, sp.w_cmd, sp.vx_std, sp.the_std = cfg.v_cmd, cfg.w_cmd, cfg.vx_std, cfg.the_std
        sp.slip_min, sp.slip_max, sp.sensor_std, sp.max_visible_dis = cfg.slip_min, cfg.slip_max, cfg.sensor_std, cfg.max_visible_dis
        sp.ticks_per_step = cfg.ticks_per_step
        w = np.ascontiguousarray(world, dtype=np.float64)
        if w.shape != (self.n, 2):
            raise ValueError("world must be [n, 2]")
        T = int(cfg.steps if steps is None else steps)
        V = int(cfg.vmax if vmax is None else vmax)
        _check(self._lib.ekf_batch_simulate_known_log(self._h, C.byref(sp), _d(w), T, V))
        self.T, self._vmax = T, V

    def download_log(self, want_truth=True):
        T, B, V, n = self.T, self.B, self._vmax, self.n
        tw, li, zz, ii = np.empty((T, B, 2)), np.empty((T, B, V), dtype=np.int32), np.empty((T, B, V, 2)), np.empty((B, 2 * n))
        tp = np.empty((T, B, 3)) if want_truth else None
        _check(self._lib.ekf_batch_download_log(self._h, _d(tw), li.ctypes.data_as(_ip), _d(zz), _d(ii),
                                                _d(tp) if want_truth else None))
        return tw, li, zz, ii, tp

    def mc_stats(self, t):
        out = np.empty(6)
        _check(self._lib.ekf_batch_mc_stats(self._h, int(t), _d(out)))
        return dict(zip(("nees_mean", "nees_max", "rmse_xy", "rmse_theta", "mean_trace_pose_cov", "frac_nees_below_95pct"), out))

    def run_known(self, t_begin=0, t_end=None, time_kernels=False):
        st = RunStats()
        _check(self._lib.ekf_batch_run_known(self._h, t_begin, self.T if t_end is None else t_end,
                                             int(time_kernels), C.byref(st)))
        return st.as_dict()

    def upload_unknown_log(self, twist, count, meas_xy):
        """twist[T,B,2], count[T,B], meas_xy[T,B,jmax,2]: prediction + data_association per step."""
        tw = np.ascontiguousarray(twist, dtype=np.float64)
        ct = np.ascontiguousarray(count, dtype=np.int32)
        me = np.ascontiguousarray(meas_xy, dtype=np.float64)
        T, B = tw.shape[0], tw.shape[1]
        if B != self.B or tw.shape != (T, B, 2) or ct.shape != (T, B) or me.ndim != 4 or me.shape[:2] != (T, B) \
                or me.shape[3] != 2:
            raise ValueError("log arrays must be twist[T,B,2], count[T,B], meas_xy[T,B,jmax,2]")
        log = UnknownLogC(T, me.shape[2], _d(tw), ct.ctypes.data_as(_ip), _d(me))
        _check(self._lib.ekf_batch_upload_unknown_log(self._h, C.byref(log)))
        self.uT, self._jmax = T, me.shape[2]

    def run_unknown(self, t_begin=0, t_end=None, time_kernels=False):
        st = RunStats()
        _check(self._lib.ekf_batch_run_unknown(self._h, t_begin, self.uT if t_end is None else t_end,
                                               int(time_kernels), C.byref(st)))
        return st.as_dict()

    @property
    def forms(self):
        f = C.c_uint()
        _check(self._lib.ekf_batch_get_forms(self._h, C.byref(f)))
        return f.value

    def set_forms(self, forms=FORMS_DEFAULT):
        """which launch structures may be taken (FORM_* bits; test / measurement hook).  What a form does to the results:

        BIT-IDENTICAL (the same operations in the same order, read from or written to another place): FORM_SMALL_MAP,
        FORM_CALL_FUSED, FORM_ACTIVE_PREFIX, FORM_STEP_FUSED, FORM_STEP_SPLIT_PASS, FORM_ROW_PACKING, FORM_TILE_QUEUE,
        FORM_STEP_CHAIN (a step's corrections in one launch, tile batch by tile batch; any set_chain setting),
        FORM_STRIP_FLUSH / _ALWAYS (strip against plain flush), FORM_STEP_SPECULATE, and the column panel -- FORM_COLUMN_PANEL
        on, off, or with FORM_COLUMN_PANEL_ONE_SLOT give the same bits in state and Sigma (tools/soak_panel.py and its slice
        in tests/test_gpu_pool_soak.py assert it, across run boundaries, getters, blind steps and sit-outs).

        EQUAL TO ROUNDING, not to the bit: FORM_CURRENT_COLUMNS (on by default).  The kept current rows / columns carry
        their rounding from launch to launch instead of being rebuilt from all pending factors: another association of the
        same sums, within 1e-10 of the rebuilt form (FORM_CURRENT_COLUMNS off) in state and, relative to its largest entry,
        in Sigma -- the bound the panel soak asserts -- and like every form within the 1e-9 contract of the eager run.
        The same holds for whatever moves a delayed flush: FORM_DELAYED_PAIR (how many corrections a launch appends), run
        boundaries and getters in mid-run, because the delayed mode's reconstruction and its flush contract their
        multiply-adds over what is pending; compare two delayed runs bit for bit only over the same
        run boundaries and the same pairing."""
        _check(self._lib.ekf_batch_set_forms(self._h, int(forms)))

    def _form(self, bit, enable):
        self.set_forms(self.forms | bit if enable else self.forms & ~bit)

    def form_counts(self):
        """covariance passes per form since creation: plain / strip flushes, paired delayed gain launches, call-fused
        passes, per-landmark rank-2 streams, step-fused launches with a separate pass, mirrored flushes, delayed gain
        launches that read the column panel"""
        c = (C.c_longlong * 8)()
        _check(self._lib.ekf_batch_form_counts(self._h, c))
        return dict(zip(("flush_plain", "flush_strip", "gain_pairs", "call_fused_passes", "rank2_streams", "step_split_passes",
                         "flush_mirrored", "gain_from_panel"), (int(x) for x in c)))

    def set_active_prefix(self, enable=True):
        self._form(FORM_ACTIVE_PREFIX, enable)

    def set_small_map_path(self, enable=True):
        self._form(FORM_SMALL_MAP, enable)

    def set_row_packing(self, enable=True):
        """narrow maps: the row-packed rank-2 kernel (default) / the plain kernel"""
        self._form(FORM_ROW_PACKING, enable)

    def set_strip_flush(self, mode="auto"):
        """delayed mode: "auto" (default: beyond 40 pending vectors on pools that fill the chip), "never", "always" """
        f = self.forms & ~(FORM_STRIP_FLUSH | FORM_STRIP_FLUSH_ALWAYS)
        self.set_forms(f | {"auto": FORM_STRIP_FLUSH, "never": 0, "always": FORM_STRIP_FLUSH | FORM_STRIP_FLUSH_ALWAYS}[mode])

    def set_known_counts(self, counts):
        """every filter's known_count (leading run of its known_list) -- the batch twin of the known_list argument"""
        c = np.ascontiguousarray(np.broadcast_to(np.asarray(counts, dtype=np.int32), (self.B,)))
        _check(self._lib.ekf_batch_set_known_counts(self._h, c.ctypes.data_as(_ip)))

    def known_counts(self):
        out = np.empty(self.B, dtype=np.int32)
        _check(self._lib.ekf_batch_get_known_counts(self._h, out.ctypes.data_as(_ip)))
        return out

    def decisions(self):
        out = np.empty((self.uT, self.B, self._jmax), dtype=np.int32)
        _check(self._lib.ekf_batch_get_decisions(self._h, out.ctypes.data_as(_ip)))
        return out

    def state(self, b):
        out = np.empty(self.N)
        _check(self._lib.ekf_batch_get_state(self._h, int(b), _d(out)))
        return out

    def cov(self, b):
        out = np.empty((self.N, self.N))
        _check(self._lib.ekf_batch_get_cov(self._h, int(b), _d(out)))
        return out

    def poses(self):
        out = np.empty((self.B, 3))
        _check(self._lib.ekf_batch_get_poses(self._h, _d(out)))
        return out

    def checksum(self):
        out = np.empty(4)
        _check(self._lib.ekf_batch_checksum(self._h, _d(out)))
        return out

    def set_tuning(self, rows_per_block=0, nontemporal=-1, group_rows=0):
        _check(self._lib.ekf_batch_set_tuning(self._h, rows_per_block, nontemporal, group_rows))

    def set_call_fused(self, enable=True):
        """every measurement() call of the pool as factor panels + ONE pass over Sigma (exact; default on); off = the
        eager per-landmark stream bench.py quotes `value` / `roofline` on"""
        self._form(FORM_CALL_FUSED, enable)

    def set_delayed_pairing(self, enable=True):
        """delayed mode: two consecutive log slots of a step per launch (default) / one launch per landmark"""
        self._form(FORM_DELAYED_PAIR, enable)

    def set_step_fused(self, enable=True):
        """unknown association beyond the LDS-resident path: True / 1 = one launch per step, two for big prefixes
        (default); 2 = always one launch; False / 0 = four launches per measurement slot"""
        e = int(enable)
        f = self.forms & ~(FORM_STEP_FUSED | FORM_STEP_SPLIT_PASS)
        self.set_forms(f | (0 if e == 0 else FORM_STEP_FUSED | (FORM_STEP_SPLIT_PASS if e == 1 else 0)))

    def rank2_packing(self):
        """P of a full-width eager correction of this pool: the rows k_rank2_packed streams as one virtual row; 1 = the
        plain kernel (the launcher and this hook read one plan, csrc/ekf_rank2_plan.hpp)"""
        P = C.c_int()
        _check(self._lib.ekf_batch_rank2_packing(self._h, C.byref(P)))
        return P.value

    def spec_counts(self):
        """(eligible, hits) of EKF_FORM_STEP_SPECULATE since creation / reset: readings of delayed unknown-association
        steps whose decision was compared with the guesses of the launch in front, and those that found their winner
        among them and continued from its rebuilt rows"""
        c = (C.c_longlong * 2)()
        _check(self._lib.ekf_batch_spec_counts(self._h, c))
        return int(c[0]), int(c[1])

    def set_step_chain(self, enable=True):
        """eager pools on the tile queue: all corrections of a step in ONE launch over Sigma (default) / one launch per
        correction"""
        self._form(FORM_STEP_CHAIN, enable)

    def set_chain(self, tiles_per_batch=0, policy=0):
        """experiment / test hook of FORM_STEP_CHAIN: tiles per queue item (0 = automatic) and the cache policy of its four
        access sets (0 = automatic; CHAIN_POLICY_EXPLICIT | bits: non-temporal where set -- 1 first loads, 2 stores of all
        sweeps but the last, 4 re-loads, 8 last stores).  Speed only: bit-identical results."""
        _check(self._lib.ekf_batch_set_chain(self._h, int(tiles_per_batch), int(policy)))

    def chain_counts(self):
        """(chained launches, correction passes they applied) since the pool was created; (0, 0) with FORM_STEP_CHAIN off"""
        c = (C.c_longlong * 2)()
        _check(self._lib.ekf_batch_chain_counts(self._h, c))
        return int(c[0]), int(c[1])

    def rank2_kernel(self):
        """name of the kernel instantiation a full-width eager correction of this pool launches (k_rank2, k_rank2_queue
        or, where rank2_packing() > 1, k_rank2_packed), + rows (packed: virtual rows) per workgroup"""
        v = [C.c_int() for _ in range(4)]
        _check(self._lib.ekf_batch_rank2_variant(self._h, *[C.byref(x) for x in v]))
        u, nt, tpb, rows = (x.value for x in v)
        if self.rank2_packing() > 1:
            return f"ekf::k_rank2_packed<{u},{'true' if nt else 'false'}>", rows
        res = C.c_int()
        _check(self._lib.ekf_batch_rank2_resident(self._h, C.byref(res)))
        return f"ekf::k_rank2{'_queue' if res.value else ''}<{u},{'true' if nt else 'false'},{tpb}>", rows

    def set_active_set(self, enable=True):
        """Stream only the rows of the touched set in the eager correction (exact; opt-in)."""
        _check(self._lib.ekf_batch_set_active_set(self._h, int(bool(enable))))

    def touched(self):
        """Per filter: how many landmarks have been corrected at least once."""
        out = np.zeros(self.B, dtype=np.int32)
        _check(self._lib.ekf_batch_get_touched(self._h, out.ctypes.data_as(_ip)))
        return out

    def set_update_mode(self, max_pending_corrections=0, symmetric_gather=False):
        """0 = eager covariance stream per correction; k > 0 = delayed rank-2k update (flush every k)."""
        _check(self._lib.ekf_batch_set_update_mode(self._h, int(max_pending_corrections), int(symmetric_gather)))


class _DensePropagatorBase:
    """What the two dense handles share; a subclass names its entry points (_PREFIX), its element type (_DTYPE) and the
    ctypes pointer to it (_PTR)."""

    def __init__(self, N, device=-1):
        self._lib = load()
        self.N = int(N)
        h = C.c_void_p()
        _check(self._entry("create")(self.N, device, C.byref(h)))
        self._h = h

    def _entry(self, name):
        return getattr(self._lib, self._PREFIX + name)

    def close(self):
        if getattr(self, "_h", None):
            self._entry("destroy")(self._h)
            self._h = None

    __del__ = close

    def _f(self, a):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=self._DTYPE)
        if a.shape != (self.N, self.N):
            raise ValueError("matrices must be N x N")
        return a, a.ctypes.data_as(self._PTR)

    def set(self, F=None, Sigma=None, Q=None):
        keep = [self._f(x) for x in (F, Sigma, Q)]
        _check(self._entry("set")(self._h, keep[0][1], keep[1][1], keep[2][1]))

    def propagate(self, iterations=1):
        ms = C.c_double()
        _check(self._entry("propagate")(self._h, int(iterations), C.byref(ms)))
        return ms.value

    @property
    def sigma(self):
        out = np.empty((self.N, self.N), dtype=self._DTYPE)
        _check(self._entry("get_sigma")(self._h, out.ctypes.data_as(self._PTR)))
        return out

    def _launch_info(self):
        v = [C.c_int() for _ in range(4)]
        _check(self._entry("launch_info")(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("ld", "tiles", "n_big", "n_tail"), (x.value for x in v)))

    def tile_map(self):
        """bool [tiles][tiles] over the 128 x 128 blocks of the result: True = computed by the tail kernel"""
        t = self.launch_info()["tiles"]
        m = np.zeros(t * t, dtype=np.uint8)
        _check(self._entry("tile_map")(self._h, m.ctypes.data_as(_bp)))
        assert set(np.unique(m)) <= {0, 1}, "a block of the result is computed by no kernel"
        return m.reshape(t, t).astype(bool)


class DensePropagator(_DensePropagatorBase):
    """Sigma <- F Sigma F^T + Q for an arbitrary dense F, fp32 on the matrix cores (configs[3]):
    the reference's `sigma = At*sigma*At.t() + Q` (ekf_slam.cpp:101-102) as two dense products."""

    _PREFIX, _DTYPE, _PTR = "ekf_dense_", np.float32, _fp

    def launch_info(self):
        """{ld, tiles, n_big, n_tail}: how one product is cut into 256 x 128 tiles and a quarter-tile tail (test hook)"""
        return self._launch_info()


class DensePropagator64(_DensePropagatorBase):
    """The fp64 twin of DensePropagator: Sigma <- F Sigma F^T + Q with fp64 operands and fp64 accumulation on the matrix
    cores, within the library's 1e-9 contract.  Takes and returns np.float64.  The handle also owns a state vector and
    the other half of a Kalman step, correct(): the measurement update for an arbitrary dense Jacobian."""

    MAX_M = 64   # EKF_DENSE64_MAX_M
    SCORE_MAX_ROWS = 2048   # EKF_DENSE64_SCORE_MAX_ROWS
    MAX_R = 64   # EKF_DENSE64_MAX_R
    MAX_S = 64   # EKF_DENSE64_MAX_S
    SCORE_SPARSE_MAX_ROWS = 65536   # EKF_DENSE64_SCORE_SPARSE_MAX_ROWS
    READ_MAX = 65536   # EKF_DENSE64_READ_MAX
    PENDING_MAX_ROWS = 64   # EKF_DENSE64_PENDING_MAX_ROWS
    LM_DEFERRED, LM_GROW_LIVE = 1, 2   # EKF_DENSE64_LM_DEFERRED, EKF_DENSE64_LM_GROW_LIVE
    LM_JOSEPH = 8   # EKF_DENSE64_LM_JOSEPH (4 stays an unknown bit)
    JOSEPH_MAX_M = 32   # EKF_DENSE64_JOSEPH_MAX_M
    SCAN_MAX_BEAMS, SCAN_MAX_CIRCLES = 1024, 128   # EKF_DENSE64_SCAN_MAX_BEAMS, EKF_DENSE64_SCAN_MAX_CIRCLES
    JOINT_MAX_READINGS, JOINT_MAX_PAIRS = 128, 30   # EKF_DENSE64_JOINT_MAX_READINGS, EKF_DENSE64_JOINT_MAX_PAIRS
    JCBB_MAX_READINGS, JCBB_MAX_CAND, JCBB_MAX_NODES = 32, 4, 1 << 22   # EKF_DENSE64_JCBB_*

    _PREFIX, _DTYPE, _PTR = "ekf_dense64_", np.float64, _dp

    @property
    def state(self):
        out = np.empty(self.N, dtype=np.float64)
        _check(self._lib.ekf_dense64_get_state(self._h, out.ctypes.data_as(_dp)))
        return out

    @state.setter
    def state(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.shape != (self.N,):
            raise ValueError("state must have length N")
        _check(self._lib.ekf_dense64_set_state(self._h, x.ctypes.data_as(_dp)))

    def correct(self, H, R, nu=None):
        """One measurement update (ekf_slam.cpp:178,186,191-192 for general operands): K = Sigma H^T (H Sigma H^T + R)^-1,
        state += K nu, Sigma <- (I - K H) Sigma.  H: m x N, R: m x m, nu: m or None (state untouched).
        Returns (nu^T S^-1 nu or None, elapsed_ms).  A singular or non-finite S raises EkfError (EKF_ERR_STATE) and
        leaves state and Sigma as they were."""
        H = np.ascontiguousarray(H, dtype=np.float64)
        if H.ndim != 2 or H.shape[1] != self.N or not 1 <= H.shape[0] <= min(self.N, self.MAX_M):
            raise ValueError(f"H must be m x N with 1 <= m <= min(N, {self.MAX_M})")
        m = H.shape[0]
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.shape != (m, m):
            raise ValueError("R must be m x m")
        nis, pnu, pnis = None, None, None
        if nu is not None:
            nu = np.ascontiguousarray(nu, dtype=np.float64)
            if nu.shape != (m,):
                raise ValueError("nu must have length m")
            nis = C.c_double()
            pnu, pnis = nu.ctypes.data_as(_dp), C.byref(nis)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_correct(self._h, m, H.ctypes.data_as(_dp), R.ctypes.data_as(_dp), pnu, pnis,
                                             C.byref(ms)))
        return (nis.value if nis is not None else None), ms.value

    def score(self, H, R, nu=None, want_S=False):
        """Score J candidate measurements without touching Sigma or the state (calculate_maha_dis, ekf_slam.cpp:217-276,
        for general operands): S_j = H_j Sigma H_j^T + R_j, nis_j = nu_j^T S_j^-1 nu_j.  H: (J, m, N); R: (m, m) shared by
        all candidates or (J, m, m); nu: (J, m) or None (no scores).  Returns (nis (J,) or None, S (J, m, m) or None,
        flags (J,) int32, elapsed_ms); a candidate whose S is singular or not finite has flag 1 and nis NaN."""
        H = np.ascontiguousarray(H, dtype=np.float64)
        if H.ndim != 3 or H.shape[2] != self.N or H.shape[0] < 1 or not 1 <= H.shape[1] <= min(self.N, self.MAX_M):
            raise ValueError(f"H must be J x m x N with J >= 1 and 1 <= m <= min(N, {self.MAX_M})")
        J, m = H.shape[0], H.shape[1]
        if J * m > self.SCORE_MAX_ROWS:
            raise ValueError(f"J * m must not exceed {self.SCORE_MAX_ROWS}")
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.shape != (m, m) and R.shape != (J, m, m):
            raise ValueError("R must be m x m or J x m x m")
        nis, S, pnu = None, None, None
        if nu is not None:
            nu = np.ascontiguousarray(nu, dtype=np.float64)
            if nu.shape != (J, m):
                raise ValueError("nu must be J x m")
            nis = np.empty(J, dtype=np.float64)
            pnu = nu.ctypes.data_as(_dp)
        if want_S:
            S = np.empty((J, m, m), dtype=np.float64)
        flags = np.empty(J, dtype=np.int32)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_score(self._h, J, m, H.ctypes.data_as(_dp), R.ctypes.data_as(_dp),
                                           1 if R.ndim == 2 else 0, pnu,
                                           nis.ctypes.data_as(_dp) if nis is not None else None,
                                           S.ctypes.data_as(_dp) if S is not None else None,
                                           flags.ctypes.data_as(_ip), C.byref(ms)))
        return nis, S, flags, ms.value

    def propagate_block(self, first, Fr, Qr=None, dx=None):
        """Block-structured prediction (ekf_slam.cpp:76-102 for a general model): Sigma <- F Sigma F^T + Q for F = identity
        with Fr in [first, first + r)^2 and Q = zero with Qr in the same square; state[first:first + r] += dx.  Fr: r x r,
        Qr: r x r or None (zero), dx: r or None (state untouched).  Only the block's rows and columns of Sigma are
        written; the F and Q given to set() play no part.  Returns elapsed_ms."""
        Fr = np.ascontiguousarray(Fr, dtype=np.float64)
        if Fr.ndim != 2 or Fr.shape[0] != Fr.shape[1] or not 1 <= Fr.shape[0] <= min(self.N, self.MAX_R):
            raise ValueError(f"Fr must be r x r with 1 <= r <= min(N, {self.MAX_R})")
        r = Fr.shape[0]
        first = int(first)
        if not 0 <= first <= self.N - r:
            raise ValueError("the block [first, first + r) must lie inside [0, N)")
        pq, pdx = None, None
        if Qr is not None:
            Qr = np.ascontiguousarray(Qr, dtype=np.float64)
            if Qr.shape != (r, r):
                raise ValueError("Qr must be r x r")
            pq = Qr.ctypes.data_as(_dp)
        if dx is not None:
            dx = np.ascontiguousarray(dx, dtype=np.float64)
            if dx.shape != (r,):
                raise ValueError("dx must have length r")
            pdx = dx.ctypes.data_as(_dp)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_propagate_block(self._h, first, r, Fr.ctypes.data_as(_dp), pq, pdx, C.byref(ms)))
        return ms.value

    def _index_lists(self, cols, ndim):
        """cols as a contiguous int32 array of `ndim` dimensions whose rows hold distinct indices in [0, N)"""
        a = np.asarray(cols)
        if a.ndim != ndim or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"cols must be an integer array of {ndim} dimension(s), not empty")
        if not 1 <= a.shape[-1] <= min(self.N, self.MAX_S):
            raise ValueError(f"cols must list s columns with 1 <= s <= min(N, {self.MAX_S})")
        if a.min() < 0 or a.max() >= self.N:
            raise ValueError("every index in cols must lie in [0, N)")
        srt = np.sort(a, axis=-1)
        if (srt[..., 1:] == srt[..., :-1]).any():
            raise ValueError("no index may appear twice in one row of cols")
        return np.ascontiguousarray(a, dtype=np.int32)

    def correct_sparse(self, cols, Hc, R, nu=None):
        """correct() for the m x N Jacobian that is zero except H[:, cols[k]] = Hc[:, k] -- the reference's Hj has five
        such columns (ekf_slam.cpp:140-178).  cols: s distinct indices in [0, N), Hc: m x s, R: m x m, nu: m or None
        (state untouched).  The panels are gathered from s rows and s columns of Sigma instead of a pass over it; every
        dot product has exactly s terms in ascending k.  Returns (nis or None, elapsed_ms); a singular or non-finite S
        raises EkfError (EKF_ERR_STATE) and leaves state and Sigma as they were."""
        return self._correct_sparse("ekf_dense64_correct_sparse", cols, Hc, R, nu)

    def correct_sparse_deferred(self, cols, Hc, R, nu=None):
        """correct_sparse() without the pass over Sigma: the same arguments, checks and results (state and nis at once,
        against the current covariance), but K and T (m rows each) are appended to the handle's pending rows instead of
        being applied.  score_sparse() and further deferred corrections read through the pending rows; flush(), or any
        other call that touches Sigma, applies them all in one pass.  With pending + m > PENDING_MAX_ROWS it flushes
        first.  A singular or non-finite S raises EkfError (EKF_ERR_STATE) and leaves state, Sigma and the pending rows."""
        return self._correct_sparse("ekf_dense64_correct_sparse_deferred", cols, Hc, R, nu)

    def correct_sparse_joseph(self, cols, Hc, R, nu=None, gain_w=None):
        """correct_sparse() in the Joseph form Sigma <- (I - K H) Sigma (I - K H)^T + K R K^T, run as Sigma - K T - D K^T
        with D = U - K S: positive semi-definite up to rounding whatever the prior against R, and valid for any gain.
        gain_w: None, or N weights in [0, 1] giving K = diag(w) U S^-1 (the partial update); a state with w = 0 is a
        consider state -- its estimate and its own block of Sigma keep their bits, its cross-covariances are updated, and
        tiles whose rows and columns are all considered are not touched.  m <= JOSEPH_MAX_M; eager only (flushes the
        pending rows first).  Returns (nis or None, tiles_skipped, elapsed_ms); a singular or non-finite S raises EkfError
        (EKF_ERR_STATE) and leaves state and Sigma as they were."""
        cols, Hc, R, nu, m, s = self._sparse_operands(cols, Hc, R, nu, self.JOSEPH_MAX_M)
        pw = None
        if gain_w is not None:
            gain_w = np.ascontiguousarray(gain_w, dtype=np.float64)
            if gain_w.shape != (self.N,):
                raise ValueError("gain_w must have length N")
            if not (np.isfinite(gain_w).all() and (gain_w >= 0.0).all() and (gain_w <= 1.0).all()):
                raise ValueError("every gain weight must be finite and in [0, 1]")
            pw = gain_w.ctypes.data_as(_dp)
        nis = C.c_double() if nu is not None else None
        skipped, ms = C.c_longlong(), C.c_double()
        _check(self._lib.ekf_dense64_correct_sparse_joseph(
            self._h, m, s, cols.ctypes.data_as(_ip), Hc.ctypes.data_as(_dp), R.ctypes.data_as(_dp),
            nu.ctypes.data_as(_dp) if nu is not None else None, pw, C.byref(nis) if nu is not None else None,
            C.byref(skipped), C.byref(ms)))
        return (nis.value if nis is not None else None), skipped.value, ms.value

    def joseph_launch_info(self):
        """{tile_rows, tile_cols, threads}: the tile of correct_sparse_joseph()'s pass over Sigma in states and its
        workgroup size (test hook)"""
        self._open()
        tr, tc, th = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_joseph_launch_info(self._h, C.byref(tr), C.byref(tc), C.byref(th)))
        return {"tile_rows": tr.value, "tile_cols": tc.value, "threads": th.value}

    def flush(self):
        """apply the pending rows to Sigma (one rank-`pending` update); a no-op with nothing pending.  Returns elapsed_ms"""
        ms = C.c_double()
        _check(self._lib.ekf_dense64_flush(self._h, C.byref(ms)))
        return ms.value

    @property
    def pending(self):
        """rows of K / T that deferred corrections have left for the flush, 0 .. PENDING_MAX_ROWS"""
        rows = C.c_int()
        _check(self._lib.ekf_dense64_pending(self._h, C.byref(rows)))
        return rows.value

    @property
    def carry(self):
        """True: propagate_block(), init_block(), swap_blocks() and sigma_block() leave the pending rows pending (the
        updates map them, the readout reads through them) and the caller chooses when to flush(); False (the default): they flush
        first.  Setting it touches nothing; it decides what the next calls do."""
        on = C.c_int()
        _check(self._lib.ekf_dense64_get_carry(self._h, C.byref(on)))
        return bool(on.value)

    @carry.setter
    def carry(self, on):
        _check(self._lib.ekf_dense64_set_carry(self._h, 1 if on else 0))

    @property
    def live(self):
        """the live dimension Na (N by default): propagate_block(), correct_sparse(), correct_sparse_deferred(),
        score_sparse(), init_block(), swap_blocks() and flush() run the filter of dimension Na in Sigma[:Na, :Na] and state[:Na], cut
        their launches for Na and neither read nor write anything at an index >= Na.  Exact when the tail is decoupled
        (coupling(Na)[0] == 0), which the reference's prior and init_block(s = 0) give.  Growing keeps the pending rows,
        shrinking flushes them first; the dense calls (propagate, correct, score, sigma, set) ignore the setting."""
        na = C.c_int()
        _check(self._lib.ekf_dense64_get_live(self._h, C.byref(na)))
        return na.value

    @live.setter
    def live(self, Na):
        _check(self._lib.ekf_dense64_set_live(self._h, int(Na)))

    def coupling(self, Na):
        """what ties Sigma[:Na, :Na] to the rest: over the entries with exactly one index >= Na, how many are != 0 and
        the largest absolute value.  Flushes first, otherwise read-only.  Returns (nonzero, max_abs, elapsed_ms)"""
        count, most, ms = C.c_longlong(), C.c_double(), C.c_double()
        _check(self._lib.ekf_dense64_coupling(self._h, int(Na), C.byref(count), C.byref(most), C.byref(ms)))
        return count.value, most.value, ms.value

    def region_begin(self, Na):
        """opens a local region A = [0, Na), 3 <= Na < N: until region_end() the structured calls run at live = Na, bit for
        bit as with live = Na, and the handle accumulates what the rest of the map owes -- exact for a COUPLED tail
        (include/ekfslam.h, ekf_dense64_region_begin).  Any call outside a region's terms ends it first.  Returns
        elapsed_ms"""
        ms = C.c_double()
        _check(self._lib.ekf_dense64_region_begin(self._h, int(Na), C.byref(ms)))
        return ms.value

    def region_end(self):
        """the global update: x_b, Sigma_bb (one MFMA product), Sigma_ba, Sigma_ab; the live dimension goes back to what
        region_begin() found.  Returns {Na, Nb, corrections, row_maps, group_bytes, elapsed_ms}"""
        rep, ms = RegionReport(), C.c_double()
        _check(self._lib.ekf_dense64_region_end(self._h, C.byref(rep), C.byref(ms)))
        out = {name: getattr(rep, name) for name, _ in RegionReport._fields_}
        out["elapsed_ms"] = ms.value
        return out

    def region_info(self):
        """{active, Na (0 without a region), corrections, row_maps (of the open region or the last one),
        ended_by_other_call (regions of this handle that a call outside their terms ended)}"""
        active, na = C.c_int(), C.c_int()
        corr, maps, ended = C.c_longlong(), C.c_longlong(), C.c_longlong()
        _check(self._lib.ekf_dense64_region_info(self._h, C.byref(active), C.byref(na), C.byref(corr), C.byref(maps),
                                                 C.byref(ended)))
        return {"active": bool(active.value), "Na": na.value, "corrections": corr.value, "row_maps": maps.value,
                "ended_by_other_call": ended.value}

    def region_launch_info(self, Na):
        """the plan of a region of Na states: {tile_rows, tile_cols, threads, pitch, update_tiles, gemm_tiles, gemm_k,
        group_bytes}"""
        v = [C.c_int() for _ in range(7)]
        b = C.c_longlong()
        _check(self._lib.ekf_dense64_region_launch_info(self._h, int(Na), *[C.byref(x) for x in v], C.byref(b)))
        names = ("tile_rows", "tile_cols", "threads", "pitch", "update_tiles", "gemm_tiles", "gemm_k")
        return {**{k: x.value for k, x in zip(names, v)}, "group_bytes": b.value}

    def padded(self):
        """test hook: (Sigma (ld, ld), state (ld,)) as they sit in memory, padding included; flushes, and ends a region"""
        ld = self.launch_info()["ld"]
        S, x = np.empty((ld, ld)), np.empty(ld)
        _check(self._lib.ekf_dense64_get_padded(self._h, S.ctypes.data_as(_dp), x.ctypes.data_as(_dp)))
        return S, x

    def region(self, Na):
        """context manager: region_begin(Na) ... region_end(); the report of the end is the manager's .report (None when a
        call inside the block ended the region first)"""
        return _Region(self, Na)

    @staticmethod
    def _r_merge(r_merge):
        r_merge = float(r_merge)
        if not (math.isfinite(r_merge) and r_merge >= 0.0):
            raise ValueError("r_merge must be finite and >= 0")
        return r_merge

    def landmark_pairs(self, n_lm, r_merge, gate=math.inf):
        """The Mahalanobis test of every pair a < b of the first n_lm landmarks (landmark i = states 3 + 2 i, 4 + 2 i) in
        one pass over Sigma's landmark corner: d2(a, b) is bit for bit the nis of score_sparse() for cols = [3 + 2a,
        4 + 2a, 3 + 2b, 4 + 2b], Hc = [[1, 0, -1, 0], [0, 1, 0, -1]], R = r_merge I, nu = x_a - x_b.  Returns (nearest
        (n_lm,) int32: the partner with the smallest score, lowest index on a tie, -1 with none; d2 (n_lm,): that score,
        +inf with none; n_below: unordered pairs with d2 < gate; n_flagged: pairs with a singular or non-finite S, which
        never win; elapsed_ms).  Flushes the pending rows first, otherwise read-only; 3 + 2 n_lm <= live."""
        n_lm, gate = int(n_lm), float(gate)
        if not 1 <= n_lm <= (self.N - 3) // 2:
            raise ValueError("1 <= n_lm <= (N - 3) // 2")
        r_merge = self._r_merge(r_merge)
        if gate != gate:
            raise ValueError("gate must not be a NaN")
        nearest, d2 = np.empty(n_lm, dtype=np.int32), np.empty(n_lm, dtype=np.float64)
        below, flagged, ms = C.c_longlong(), C.c_longlong(), C.c_double()
        _check(self._lib.ekf_dense64_score_landmark_pairs(self._h, n_lm, r_merge, gate, nearest.ctypes.data_as(_ip),
                                                          d2.ctypes.data_as(_dp), C.byref(below), C.byref(flagged),
                                                          C.byref(ms)))
        return nearest, d2, below.value, flagged.value, ms.value

    def pairs_launch_info(self):
        """{tile_landmarks, threads}: the side of landmark_pairs()' tiles in landmarks and its workgroup size (test hook)"""
        tl, th = C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_pairs_launch_info(self._h, C.byref(tl), C.byref(th)))
        return {"tile_landmarks": tl.value, "threads": th.value}

    def merge_landmarks(self, a, b, r_merge, known, flags=0, params=None):
        """Fuse landmarks a and b (either order) of the `known` ones and remove the higher: correct_sparse() -- with
        LM_DEFERRED in flags correct_sparse_deferred() -- on landmark_pairs()' operands for (min, max), built on the
        device; then swap_blocks(max, last) unless max is the last, init_block(last, W = sigma0 I) and known - 1; with
        LM_GROW_LIVE also live = 3 + 2 known, with LM_JOSEPH correct_sparse_joseph().  Bit for bit that sequence spelled.  Returns (known, moved_from: the old index
        of the landmark that now sits in slot max, or -1; d2: the correction's nis; elapsed_ms).  A singular S raises
        EkfError (EKF_ERR_STATE) and leaves everything as it was."""
        a, b, known, flags = int(a), int(b), int(known), int(flags)
        if not 0 <= known <= (self.N - 3) // 2:
            raise ValueError("0 <= known <= (N - 3) // 2")
        if a == b or not (0 <= a < known and 0 <= b < known):
            raise ValueError("a and b must be two different landmarks in [0, known)")
        r_merge = self._r_merge(r_merge)
        if flags & ~(self.LM_DEFERRED | self.LM_GROW_LIVE | self.LM_JOSEPH) or \
                (flags & self.LM_JOSEPH and flags & self.LM_DEFERRED):
            raise ValueError("flags: LM_DEFERRED | LM_GROW_LIVE | LM_JOSEPH, the last not with the first")
        k, moved, d2, ms = C.c_int(known), C.c_int(-1), C.c_double(), C.c_double()
        _check(self._lib.ekf_dense64_merge_landmarks(self._h, C.byref(params) if params is not None else None, a, b, r_merge,
                                                     C.byref(k), flags, C.byref(moved), C.byref(d2), C.byref(ms)))
        return k.value, moved.value, d2.value, ms.value

    def remove_landmark(self, i, known, flags=0, params=None):
        """Remove landmark i of the `known` ones, the removal half of merge_landmarks(): swap_blocks(i, last) unless i is
        the last, init_block(last, W = sigma0 I) and known - 1; with LM_GROW_LIVE (the only flag) also live = 3 + 2 known.
        Bit for bit that sequence spelled.  Returns (known, moved_from: the old index of the landmark that now sits in
        slot i, or -1; elapsed_ms)."""
        i, known, flags = int(i), int(known), int(flags)
        if not 0 <= known <= (self.N - 3) // 2:
            raise ValueError("0 <= known <= (N - 3) // 2")
        if not 0 <= i < known:
            raise ValueError("i must be a landmark in [0, known)")
        if flags & ~self.LM_GROW_LIVE:
            raise ValueError("flags: LM_GROW_LIVE")
        k, moved, ms = C.c_int(known), C.c_int(-1), C.c_double()
        _check(self._lib.ekf_dense64_remove_landmark(self._h, C.byref(params) if params is not None else None, i,
                                                     C.byref(k), flags, C.byref(moved), C.byref(ms)))
        return k.value, moved.value, ms.value

    def evidence_launch_info(self):
        """{beam_tile, lm_chunk, threads}: the beams of a workgroup of scan_evidence(), the candidates it stages in LDS at
        a time and its workgroup size (test hook)"""
        self._open()
        bt, lc, th = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_evidence_launch_info(self._h, C.byref(bt), C.byref(lc), C.byref(th)))
        return {"beam_tile": bt.value, "lm_chunk": lc.value, "threads": th.value}

    def scan_evidence(self, ranges, lidar=None, first_lm=0, count=None, tol_abs=0.05, kappa=2.0, params=None):
        """One scan cast against the handle's own map (ekf_dense64_scan_evidence, include/ekfslam.h): per beam the range
        the landmarks [first_lm, first_lm + count) predict (clean ray geometry of `lidar`, default_lidar() if None) and
        the landmark it should stop on; per landmark how many of its beams agree with `ranges`, went through it, stopped
        short of it, under tol = tol_abs + kappa sqrt(range variance of the landmark under Sigma).  ranges None: the
        expected scan only (lidar.n_beams beams).  count None: every landmark from first_lm inside the live dimension.
        Read-only, nothing is flushed.  Returns a ScanEvidence."""
        self._open()
        lp = lidar if lidar is not None else default_lidar()
        if ranges is not None:
            r = self._scan(ranges)
            if r.shape[0] != lp.n_beams:
                if lidar is not None:
                    raise ValueError("ranges must hold lidar.n_beams beams")
                lp.n_beams = r.shape[0]
        first_lm, count = self._value_range(first_lm, count)
        n, nb = max(count, 0), max(min(int(lp.n_beams), self.SCAN_MAX_BEAMS), 0)
        ne, na, nt, ns = (np.zeros(n, dtype=np.int32) for _ in range(4))
        tol, exp = np.empty(n, dtype=np.float64), np.empty(nb, dtype=np.float64)
        hit, cls = np.empty(nb, dtype=np.int32), np.empty(nb, dtype=np.uint8)
        rep, ms = EvidenceReport(), C.c_double()
        _check(self._lib.ekf_dense64_scan_evidence(
            self._h, C.byref(params) if params is not None else None, C.byref(lp), _d(r) if ranges is not None else None,
            first_lm, count, float(tol_abs), float(kappa), ne.ctypes.data_as(_ip), na.ctypes.data_as(_ip),
            nt.ctypes.data_as(_ip), ns.ctypes.data_as(_ip), _d(tol), _d(exp), hit.ctypes.data_as(_ip),
            cls.ctypes.data_as(_bp), C.byref(rep), C.byref(ms)))
        return ScanEvidence(first_lm, ne, na, nt, ns, tol, exp, hit, cls, rep, ms.value)

    def _open(self):
        if not getattr(self, "_h", None):
            raise ValueError("the handle is closed")

    def health(self):
        """Is Sigma[:live, :live] still a covariance?  One read-only pass on the device (ekf_dense64_health_report,
        include/ekfslam.h): n_nonfinite (NaN or Inf entries), n_asym (pairs i < j whose two entries differ in bits),
        max_asym / asym_i / asym_j (the largest |Sigma[i][j] - Sigma[j][i]| on its bit pattern, so a NaN wins, and the
        lowest (i, j) that attains it; 0.0, -1, -1 with no pair), min_diag / min_diag_i (the smallest diagonal entry that
        is not a NaN, lowest index on equal values; +inf, -1 with none), n_diag_bad (diagonal entries NaN or <= 0),
        n_minor (pairs with Sigma[i][j] Sigma[j][i] > Sigma[i][i] Sigma[j][j]) and ms.  Flushes the pending rows first."""
        self._open()
        rep, ms = HealthReport(), C.c_double()
        _check(self._lib.ekf_dense64_health(self._h, C.byref(rep), C.byref(ms)))
        out = {name: getattr(rep, name) for name, _ in HealthReport._fields_ if name != "reserved"}
        out["ms"] = ms.value
        return out

    def symmetrize(self):
        """Sigma[i][j] = Sigma[j][i] = 0.5 * (Sigma[i][j] + Sigma[j][i]) for every pair i < j < live whose two entries
        differ in bits, in place on the device; equal pairs and the diagonal are not written.  Flushes the pending rows
        first.  Returns {changed: the pairs written, max_asym: as health()'s before the call, ms}"""
        self._open()
        changed, most, ms = C.c_longlong(), C.c_double(), C.c_double()
        _check(self._lib.ekf_dense64_symmetrize(self._h, C.byref(changed), C.byref(most), C.byref(ms)))
        return {"changed": changed.value, "max_asym": most.value, "ms": ms.value}

    def health_launch_info(self):
        """{tile, threads}: the side of health()'s and symmetrize()'s tiles in states and their workgroup size (test hook)"""
        self._open()
        tile, th = C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_health_launch_info(self._h, C.byref(tile), C.byref(th)))
        return {"tile": tile.value, "threads": th.value}

    def value_launch_info(self):
        """{tile_rows, tile_lm, threads}: the tile of value_operands()' and rank_landmarks()' pass over Sigma -- tile_rows
        fixes the order of their sums -- and its workgroup size (test hook)"""
        self._open()
        tr, tl, th = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_value_launch_info(self._h, C.byref(tr), C.byref(tl), C.byref(th)))
        return {"tile_rows": tr.value, "tile_lm": tl.value, "threads": th.value}

    def _value_range(self, first_lm, count):
        first_lm = int(first_lm)
        if count is None:
            count = (self.live - 3) // 2 - first_lm
        return first_lm, int(count)

    def value_operands(self, Hc, R, first_lm=0, in_view=None):
        """What one observation of each landmark in [first_lm, first_lm + count) would gain, for Jacobians given by the
        caller: Hc (count, 2, 5) on the columns {0, 1, 2, 3 + 2 i, 4 + 2 i}, R (2, 2) shared; in_view (count,) or None
        (all) gates the winners only.  One read-only pass over Sigma[:live, :live] for all of them (ekf_dense64_value_operands,
        include/ekfslam.h); flushes the pending rows first.  Returns an ObservationValue."""
        self._open()
        Hc = np.ascontiguousarray(Hc, dtype=np.float64)
        R = np.ascontiguousarray(R, dtype=np.float64)
        if Hc.ndim != 3 or Hc.shape[1:] != (2, 5) or R.shape != (2, 2):
            raise ValueError("Hc must be count x 2 x 5 and R 2 x 2")
        first_lm, count = self._value_range(first_lm, Hc.shape[0])
        if in_view is not None:
            in_view = np.ascontiguousarray(in_view, dtype=np.uint8)
            if in_view.shape != (count,):
                raise ValueError("in_view must hold count entries")
        n = max(count, 0)
        dt, dp, det = (np.empty(n, dtype=np.float64) for _ in range(3))
        S, flags = np.empty((n, 2, 2), dtype=np.float64), np.empty(n, dtype=np.int32)
        best, ms = ValueBest(), C.c_double()
        _check(self._lib.ekf_dense64_value_operands(
            self._h, first_lm, count, _d(Hc), _d(R), in_view.ctypes.data_as(_bp) if in_view is not None else None,
            _d(dt), _d(dp), _d(det), _d(S), flags.ctypes.data_as(_ip), C.byref(best), C.byref(ms)))
        view = in_view if in_view is not None else np.ones(n, dtype=np.uint8)
        return ObservationValue(first_lm, dt, dp, det, S, flags, view, Hc, R, best, ms.value)

    def rank_landmarks(self, first_lm=0, count=None, range_max=None, params=None):
        """value_operands() with the reference's measurement model on the handle's own state [theta, x, y, m1x, m1y, ...]:
        Hc is Hj of measurement() for each landmark (score_landmarks()' Hc, bit for bit), R = r_meas I, and in_view =
        (predicted range <= range_max), everything in view with range_max None.  count None: every landmark from first_lm
        that lies inside the live dimension.  Nothing goes up and only the results come down.  Returns an
        ObservationValue."""
        self._open()
        first_lm, count = self._value_range(first_lm, count)
        n = max(count, 0)
        dt, dp, det = (np.empty(n, dtype=np.float64) for _ in range(3))
        S, flags = np.empty((n, 2, 2), dtype=np.float64), np.empty(n, dtype=np.int32)
        view, Hc = np.empty(n, dtype=np.uint8), np.empty((n, 2, 5), dtype=np.float64)
        best, ms = ValueBest(), C.c_double()
        _check(self._lib.ekf_dense64_rank_landmarks(
            self._h, C.byref(params) if params is not None else None, first_lm, count,
            0.0 if range_max is None else float(range_max), _d(dt), _d(dp), _d(det), _d(S), flags.ctypes.data_as(_ip),
            C.byref(best), view.ctypes.data_as(_bp), _d(Hc), C.byref(ms)))
        r = (params if params is not None else default_params()).r_meas
        return ObservationValue(first_lm, dt, dp, det, S, flags, view, Hc, r * np.eye(2), best, ms.value)

    WHITEN_MAX_RHS = 64   # EKF_DENSE64_WHITEN_MAX_RHS

    def factor(self):
        """The Cholesky factor L of Sigma[:live, :live] (its lower triangle: Sigma[i][j], j <= i), taken on the device into
        a snapshot buffer of the handle's own; Sigma and the state are only read.  Flushes the pending rows first.  Returns
        ekf_dense64_factor_report (include/ekfslam.h) as a dict: ok (1: Sigma is positive definite), fail_index / fail_pivot
        (the first column whose pivot was not finite and > 0), min_pivot / max_pivot / min_pivot_i (of L[j][j]^2 over the
        columns factored), Na, logdet (log det Sigma summed on the host; NaN unless ok) and ms."""
        self._open()
        rep, ms = FactorReport(), C.c_double()
        _check(self._lib.ekf_dense64_factor(self._h, C.byref(rep), C.byref(ms)))
        out = {name: getattr(rep, name) for name, _ in FactorReport._fields_}
        out["ms"] = ms.value
        self._factor_na = rep.Na
        return out

    def get_factor(self):
        """L of the last factor(), Na x Na (the live dimension it was taken at) with an exactly zero strict upper triangle:
        the snapshot as taken, whatever has happened to Sigma or the live dimension since.  EkfError (EKF_ERR_STATE) before
        the first factor() and after one that ended with ok == 0."""
        self._open()
        Na = getattr(self, "_factor_na", None) or 1   # (before the first factor the library refuses and writes nothing)
        out = np.empty((Na, Na), dtype=np.float64)
        _check(self._lib.ekf_dense64_get_factor(self._h, _d(out)))
        return out

    def whiten(self, B, want_Y=True):
        """Y[r] = L^-1 B[r] by forward substitution against the last factor() and d2[r] = |Y[r]|^2 for the rows of B
        (nrhs x live, or one vector), up to WHITEN_MAX_RHS at once; with B = state - truth d2 is the NEES of the whole map.
        Does not read Sigma and does not flush the pending rows.  Returns {Y (None unless want_Y), d2, ms}."""
        B = self._rhs(B, "B")
        Y = np.empty_like(B) if want_Y else None
        d2, ms = np.empty(B.shape[0]), C.c_double()
        _check(self._lib.ekf_dense64_whiten(self._h, B.shape[0], _d(B), _d(Y) if want_Y else None, _d(d2), C.byref(ms)))
        return {"Y": Y, "d2": d2, "ms": ms.value}

    def _rhs(self, B, name):
        """the argument checks of whiten(), solve() and color(): nrhs x live (or one vector), C-contiguous float64"""
        self._open()
        B = np.ascontiguousarray(B, dtype=np.float64)
        if B.ndim == 1:
            B = B[None, :]
        if B.ndim != 2 or not 1 <= B.shape[0] <= self.WHITEN_MAX_RHS or B.shape[1] != self.live:
            raise ValueError(f"{name} must be nrhs x live with 1 <= nrhs <= {self.WHITEN_MAX_RHS}")
        return B

    def solve(self, B, want_Y=False):
        """X[r] = Sigma^-1 B[r] = L^-T (L^-1 B[r]) against the last factor(), for the rows of B (nrhs x live, or one
        vector), up to WHITEN_MAX_RHS at once: whiten()'s forward substitution as it stands (Y and d2 are whiten()'s bit
        for bit), then the backward substitution, descending, divisions by L[i][i].  Does not read Sigma and does not flush
        the pending rows.  Returns {X, Y (None unless want_Y), d2, ms}."""
        B = self._rhs(B, "B")
        X = np.empty_like(B)
        Y = np.empty_like(B) if want_Y else None
        d2, ms = np.empty(B.shape[0]), C.c_double()
        _check(self._lib.ekf_dense64_solve(self._h, B.shape[0], _d(B), _d(X), _d(Y) if want_Y else None, _d(d2), C.byref(ms)))
        return {"X": X, "Y": Y, "d2": d2, "ms": ms.value}

    def color(self, Z, add_state=False):
        """X[r] = L Z[r] against the last factor(), for the rows of Z (nrhs x live, or one vector), up to WHITEN_MAX_RHS at
        once; with add_state X[r] = fl(L Z[r] + state[:live]), the CURRENT state: rows of unit normal draws become maps
        drawn from N(state, Sigma of the last factor()).  The heading of a sample is not wrapped.  Does not read Sigma and
        does not flush the pending rows.  Returns {X, ms}."""
        Z = self._rhs(Z, "Z")
        X, ms = np.empty_like(Z), C.c_double()
        _check(self._lib.ekf_dense64_color(self._h, Z.shape[0], _d(Z), 1 if add_state else 0, _d(X), C.byref(ms)))
        return {"X": X, "ms": ms.value}

    def solve_launch_info(self):
        """{block, threads_back, threads_color}: the block side of solve() and color() in states and the workgroup sizes of
        the backward step and of the colouring kernel (test hook)"""
        self._open()
        block, tb, tc = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_solve_launch_info(self._h, C.byref(block), C.byref(tb), C.byref(tc)))
        return {"block": block.value, "threads_back": tb.value, "threads_color": tc.value}

    def factor_launch_info(self):
        """{block, threads}: the block side of factor() in states and the workgroup size (test hook)"""
        self._open()
        block, th = C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_factor_launch_info(self._h, C.byref(block), C.byref(th)))
        return {"block": block.value, "threads": th.value}

    FRAME_FIXED, FRAME_ROBOT = 0, 1   # EKF_DENSE64_FRAME_FIXED, EKF_DENSE64_FRAME_ROBOT

    def map_congruence(self, G, C=None):
        """Sigma[:live, :live] <- J Sigma J^T in place for J = blockdiag(1, G, ..., G) + [C | 0] (ekf_dense64_map_congruence,
        include/ekfslam.h): G 2 x 2 on the robot position and every landmark (the pairs (1, 2), (3, 4), ...), C live x 3 on
        the pose columns or None (the rank-6 part is skipped; with G = I in bits Sigma is not passed over).  live must be
        3 + 2 n.  Flushes the pending rows first; the state is not touched; Sigma is never symmetrised.  Returns elapsed_ms"""
        self._open()
        G = np.ascontiguousarray(G, dtype=np.float64)
        if G.shape != (2, 2):
            raise ValueError("G must be 2 x 2")
        if C is not None:
            C = np.ascontiguousarray(C, dtype=np.float64)
            if C.shape != (self.live, 3):
                raise ValueError("C must be live x 3")
        ms = np.zeros(1)   # (the parameter C hides ctypes here)
        _check(self._lib.ekf_dense64_map_congruence(self._h, _d(G), _d(C) if C is not None else None, _d(ms)))
        return float(ms[0])

    def reframe(self, mode, dtheta=0.0, tx=0.0, ty=0.0, want_terms=False):
        """State and Sigma of the live corner into another frame (ekf_dense64_reframe_landmarks).  FRAME_FIXED: theta +=
        dtheta (not wrapped), q <- R(dtheta) q + (tx, ty) for the robot position and every landmark.  FRAME_ROBOT: the map in
        the robot's own frame, the old origin becomes the "pose" (dtheta, tx, ty ignored); its own inverse up to rounding,
        and until it is called again the state is not what predict_landmarks() assumes.  Returns elapsed_ms, or with
        want_terms (True, or a float64 vector of at least 4 + 3 live entries to fill) (G (2, 2), C (live, 3) or None for FRAME_FIXED, elapsed_ms): map_congruence(G, C) gives the same Sigma
        bit for bit."""
        self._open()
        mode = int(mode)
        terms = None
        if isinstance(want_terms, np.ndarray):   # the caller's own buffer: the library writes 4 + 3 live doubles into it
            terms = want_terms
            if terms.dtype != np.float64 or terms.ndim != 1 or not terms.flags.c_contiguous or terms.shape[0] < 4 + 3 * self.live:
                raise ValueError("terms must be a contiguous float64 vector of at least 4 + 3 live entries")
        elif want_terms:
            terms = np.empty(4 + 3 * self.live, dtype=np.float64)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_reframe_landmarks(self._h, mode, float(dtheta), float(tx), float(ty),
                                                       _d(terms) if terms is not None else None, C.byref(ms)))
        if terms is None:
            return ms.value
        terms = terms[:4 + 3 * self.live]
        return terms[:4].reshape(2, 2).copy(), (terms[4:].reshape(-1, 3).copy() if mode == self.FRAME_ROBOT else None), ms.value

    def frame_launch_info(self):
        """{tile_rows, tile_cols, threads}: the tile of map_congruence()'s pass in states (origins at 3 + a tile_rows,
        3 + b tile_cols) and its workgroup size (test hook)"""
        self._open()
        tr, tc, th = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_frame_launch_info(self._h, C.byref(tr), C.byref(tc), C.byref(th)))
        return {"tile_rows": tr.value, "tile_cols": tc.value, "threads": th.value}

    def _join_source(self, src):
        self._open()
        if not isinstance(src, DensePropagator64):
            raise ValueError("the source must be a DensePropagator64")
        src._open()
        return src

    def join_congruence(self, src, G, E):
        """The covariance of src's live corner (Nb states) joined onto this handle's (ekf_dense64_join_congruence,
        include/ekfslam.h): Y = D Sigma_B D^T + E Sigma_pp E^T at the indices 0, 1, 2, live, live + 1, ..., the cross terms
        E P and Pc E^T beside it; Sigma[3:live, 3:live] is not touched and src is read only.  G 2 x 2, E Nb x 3, every
        entry multiplied through.  Both live dimensions must be 3 + 2 n.  Flushes the pending rows of both handles; touches
        neither state; afterwards live is live + Nb - 3.  Returns elapsed_ms"""
        src = self._join_source(src)
        G = np.ascontiguousarray(G, dtype=np.float64)
        E = np.ascontiguousarray(E, dtype=np.float64)
        if G.shape != (2, 2):
            raise ValueError("G must be 2 x 2")
        if src.region_info()["active"]:   # (the library would end it and take the live dimension behind it: E could not be checked)
            raise ValueError("the source is inside a local region: end it before join_congruence()")
        if E.shape != (src.live, 3):
            raise ValueError("E must be (the source's live) x 3")
        ms = C.c_double()
        _check(self._lib.ekf_dense64_join_congruence(self._h, src._h, _d(G), _d(E), C.byref(ms)))
        return ms.value

    def join_map(self, src, want_terms=False):
        """Map joining (ekf_dense64_join_map): src holds a local map in the frame of this handle's robot pose, independent
        of this map (started at pose 0 with zero pose covariance -- the caller's duty).  The pose becomes the composition
        (theta not wrapped), src's landmarks are appended in this frame at the states live, live + 1, ..., Sigma as
        join_congruence() with G and E built on the device.  src keeps its state, its Sigma and its live dimension.
        Returns elapsed_ms, or with want_terms (G (2, 2), E (Nb, 3), elapsed_ms): join_congruence(src, G, E) gives the same
        Sigma bit for bit."""
        src = self._join_source(src)
        terms = np.empty(4 + 3 * src.N, dtype=np.float64) if want_terms else None   # (a region src is in ends: Nb <= N)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_join_map(self._h, src._h, _d(terms) if want_terms else None, C.byref(ms)))
        if not want_terms:
            return ms.value
        Nb = src.live
        return terms[:4].reshape(2, 2).copy(), terms[4:4 + 3 * Nb].reshape(Nb, 3).copy(), ms.value

    def join_launch_info(self):
        """{tile_rows, tile_cols, threads}: the tile of the join's pass over the source's Sigma[3:Nb, 3:Nb] in states
        (origins at 3 + a tile_rows, 3 + b tile_cols) and its workgroup size (test hook)"""
        self._open()
        tr, tc, th = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_join_launch_info(self._h, C.byref(tr), C.byref(tc), C.byref(th)))
        return {"tile_rows": tr.value, "tile_cols": tc.value, "threads": th.value}

    def extract_map(self, src, keep=None):
        """This handle becomes a copy of src's map, or of a submap of it (ekf_dense64_extract_map, include/ekfslam.h): the
        pose and the landmarks keep[0], keep[1], ... of src (distinct, any order; None: all of them in order, a clone), by
        Sigma[i][j] = Sigma_src[iota(i)][iota(j)] and state[i] = state_src[iota(i)] with iota(3 + 2 t + c) = 3 + 2 keep[t] + c,
        every bit kept.  live becomes 3 + 2 len(keep); nothing at an index from it on is touched.  src's pending rows are
        carried into this handle, not applied, and src is unchanged (an open region on it ends first); this handle's own
        pending rows are applied and its region is ended first.  Returns elapsed_ms"""
        src = self._join_source(src)
        if src is self:
            raise ValueError("extract_map() is out of place: the source must be another handle")
        if keep is None:
            ms = C.c_double()
            _check(self._lib.ekf_dense64_extract_map(self._h, src._h, -1, None, C.byref(ms)))
            return ms.value
        a = np.asarray(keep)
        if a.ndim != 1 or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
            raise ValueError("keep must be a list of landmark indices (one dimension, integers)")
        a = np.ascontiguousarray(a, dtype=np.int64)
        if a.size and a.min() < 0:
            raise ValueError("every index of keep must be a landmark of the source, in [0, b)")
        if np.unique(a).size != a.size:
            raise ValueError("keep names a landmark twice")
        if 3 + 2 * a.size > self.N:
            raise ValueError(f"3 + 2 * {a.size} states do not fit N = {self.N}")
        if src.region_info()["active"]:   # (the library would end it and take the live dimension behind it: keep could not be checked)
            raise ValueError("the source is inside a local region: end it before extract_map() with a list")
        b = (src.live - 3) // 2
        if a.size and a.max() >= b:
            raise ValueError(f"every index of keep must be a landmark of the source, in [0, {b})")
        k = int(a.size)
        a = np.ascontiguousarray(a if k else [0], dtype=np.int32)   # (an empty list is still a list: never a null pointer)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_extract_map(self._h, src._h, k, a.ctypes.data_as(_ip), C.byref(ms)))
        return ms.value

    def extract_launch_info(self):
        """{tile_rows, tile_cols, threads}: the tile of extract_map()'s pass over this handle's Sigma[3:Nd, 3:Nd] in states
        (origins at 3 + a tile_rows, 3 + b tile_cols) and its workgroup size (test hook)"""
        self._open()
        tr, tc, th = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_extract_launch_info(self._h, C.byref(tr), C.byref(tc), C.byref(th)))
        return {"tile_rows": tr.value, "tile_cols": tc.value, "threads": th.value}

    def _sparse_operands(self, cols, Hc, R, nu, max_m):
        """the shape and range checks of a sparse correction -> (cols int32, Hc, R, nu or None, m, s), contiguous"""
        cols = self._index_lists(cols, 1)
        s = cols.shape[0]
        Hc = np.ascontiguousarray(Hc, dtype=np.float64)
        if Hc.ndim != 2 or Hc.shape[1] != s or not 1 <= Hc.shape[0] <= min(self.N, max_m):
            raise ValueError(f"Hc must be m x s with 1 <= m <= min(N, {max_m})")
        m = Hc.shape[0]
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.shape != (m, m):
            raise ValueError("R must be m x m")
        if nu is not None:
            nu = np.ascontiguousarray(nu, dtype=np.float64)
            if nu.shape != (m,):
                raise ValueError("nu must have length m")
        return cols, Hc, R, nu, m, s

    def _correct_sparse(self, entry, cols, Hc, R, nu):
        cols, Hc, R, nu, m, s = self._sparse_operands(cols, Hc, R, nu, self.MAX_M)
        nis, pnu, pnis = None, None, None
        if nu is not None:
            nis = C.c_double()
            pnu, pnis = nu.ctypes.data_as(_dp), C.byref(nis)
        ms = C.c_double()
        _check(getattr(self._lib, entry)(self._h, m, s, cols.ctypes.data_as(_ip), Hc.ctypes.data_as(_dp), R.ctypes.data_as(_dp), pnu, pnis,
                    C.byref(ms)))
        return (nis.value if nis is not None else None), ms.value

    def score_sparse(self, cols, Hc, R, nu=None, want_S=False):
        """score() for J Jacobians given by their non-zero columns: H_j is zero except H_j[:, cols[j, k]] = Hc[j, :, k].
        cols: (J, s) with distinct indices in every row, Hc: (J, m, s); R: (m, m) shared or (J, m, m); nu: (J, m) or None.
        Only the s x s blocks Sigma[cols_j, cols_j] are read, in one launch; J * m may reach SCORE_SPARSE_MAX_ROWS, so a
        reading is scored against every landmark of a full map in one call.  Returns what score() returns."""
        cols = self._index_lists(cols, 2)
        J, s = cols.shape
        Hc = np.ascontiguousarray(Hc, dtype=np.float64)
        if Hc.ndim != 3 or Hc.shape[0] != J or Hc.shape[2] != s or not 1 <= Hc.shape[1] <= min(self.N, self.MAX_M):
            raise ValueError(f"Hc must be J x m x s with 1 <= m <= min(N, {self.MAX_M})")
        m = Hc.shape[1]
        if J * m > self.SCORE_SPARSE_MAX_ROWS:
            raise ValueError(f"J * m must not exceed {self.SCORE_SPARSE_MAX_ROWS}")
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.shape != (m, m) and R.shape != (J, m, m):
            raise ValueError("R must be m x m or J x m x m")
        nis, S, pnu = None, None, None
        if nu is not None:
            nu = np.ascontiguousarray(nu, dtype=np.float64)
            if nu.shape != (J, m):
                raise ValueError("nu must be J x m")
            nis = np.empty(J, dtype=np.float64)
            pnu = nu.ctypes.data_as(_dp)
        if want_S:
            S = np.empty((J, m, m), dtype=np.float64)
        flags = np.empty(J, dtype=np.int32)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_score_sparse(self._h, J, m, s, cols.ctypes.data_as(_ip), Hc.ctypes.data_as(_dp),
                                                  R.ctypes.data_as(_dp), 1 if R.ndim == 2 else 0, pnu,
                                                  nis.ctypes.data_as(_dp) if nis is not None else None,
                                                  S.ctypes.data_as(_dp) if S is not None else None,
                                                  flags.ctypes.data_as(_ip), C.byref(ms)))
        return nis, S, flags, ms.value

    def score_landmarks(self, sx, sy, first_lm=0, count=None, want_S=False, want_terms=False, params=None):
        """calculate_maha_dis (ekf_slam.cpp:217-276) of the reading (sx, sy) against landmarks [first_lm, first_lm + count)
        of the handle's own state [theta, x, y, m1x, m1y, ...]: the operands are built on the device and scored by
        score_sparse()'s kernel, read-only.  count None: every landmark from first_lm that lies inside the live dimension.
        params: a Params or None (the reference's constants).  Returns (nis, S or None, flags, elapsed_ms), and with
        want_terms also (cols (count, 5), Hc (count, 2, 5), nu (count, 2) raw) -- handed back to score_sparse() they give
        the same bits."""
        first_lm = int(first_lm)
        if count is None:
            count = (self.live - 3) // 2 - first_lm
        count = int(count)
        if first_lm < 0 or not 1 <= count <= self.SCORE_SPARSE_MAX_ROWS // 2:
            raise ValueError(f"first_lm >= 0 and 1 <= count <= {self.SCORE_SPARSE_MAX_ROWS // 2}")
        nis, flags = np.empty(count, dtype=np.float64), np.empty(count, dtype=np.int32)
        S = np.empty((count, 2, 2), dtype=np.float64) if want_S else None
        cols = np.empty((count, 5), dtype=np.int32) if want_terms else None
        Hc = np.empty((count, 2, 5), dtype=np.float64) if want_terms else None
        nu = np.empty((count, 2), dtype=np.float64) if want_terms else None
        ms = C.c_double()
        _check(self._lib.ekf_dense64_score_landmarks(
            self._h, C.byref(params) if params is not None else None, float(sx), float(sy), first_lm, count,
            nis.ctypes.data_as(_dp), S.ctypes.data_as(_dp) if want_S else None, flags.ctypes.data_as(_ip),
            cols.ctypes.data_as(_ip) if want_terms else None, Hc.ctypes.data_as(_dp) if want_terms else None,
            nu.ctypes.data_as(_dp) if want_terms else None, C.byref(ms)))
        if want_terms:
            return nis, S, flags, ms.value, (cols, Hc, nu)
        return nis, S, flags, ms.value

    def _lm_flags(self, deferred, grow_live=False, joseph=False):
        if deferred and joseph:
            raise ValueError("joseph is an eager form: not with deferred")
        return (self.LM_DEFERRED if deferred else 0) | (self.LM_GROW_LIVE if grow_live else 0) | \
               (self.LM_JOSEPH if joseph else 0)

    def _jcbb_args(self, jcbb, n, per, params):
        """jcbb = (gate_ic, gate_joint, max_nodes) of a jcbb association call for up to n readings -> (the three arguments in
        front of the flags (the pointer keeps its array), the report behind best); None, the other rules -> ([], None)"""
        if jcbb is None:
            return [], None
        gate_ic, gate_joint, max_nodes = jcbb
        g = None if gate_joint is None else np.ascontiguousarray(gate_joint, dtype=np.float64)
        if g is not None and g.shape != (n,):
            raise ValueError(f"gate_joint must hold one gate per {per}")
        return [self._gate_ic(gate_ic, params), g.ctypes.data_as(_dp) if g is not None else None, int(max_nodes)], JcbbReport()

    def _associate_readings(self, call, z, known, n_max, deferred, grow_live, params, joseph=False, jcbb=None, groups=True):
        """The readings form of the three association rules: the C call named `call` on z (J, 2), checked by the caller.
        jcbb: (gate_ic, gate_joint, max_nodes) for that rule, whose call also fills a report; groups: the call has
        n_groups_out.  Returns (known, assoc (J,), best (J,), report or None, n_groups, elapsed_ms); an EkfError carries
        .known, .assoc, .best and that rule's .report as they stood."""
        J = z.shape[0]
        k, ng, ms = C.c_int(int(known)), C.c_int(0), C.c_double()
        assoc, best = np.full(J, -2, dtype=np.int32), np.empty(J, dtype=np.float64)
        gates, rep = self._jcbb_args(jcbb, J, "reading", params)
        flags = self._lm_flags(deferred, grow_live, joseph)
        tail = [C.byref(o) for o in (rep, ng if groups else None, ms) if o is not None]
        try:
            _check(getattr(self._lib, call)(
                self._h, C.byref(params) if params is not None else None, J, z.ctypes.data_as(_dp), int(n_max), C.byref(k),
                *gates, flags, assoc.ctypes.data_as(_ip), best.ctypes.data_as(_dp), *tail))
        except EkfError as e:
            e.known, e.assoc, e.best = k.value, assoc, best
            if rep is not None:
                e.report = rep.as_dict()
            raise
        return k.value, assoc, best, rep, ng.value, ms.value

    def _associate_scan(self, call, ranges, max_readings, most, known, n_max, deferred, grow_live, params, jcbb=None):
        """The scan form of the three association rules: the C call named `call` on one scan and at most max_readings <= most
        of its circles.  jcbb as in _associate_readings.  Returns (known, centres (k, 2), assoc (k,), best (k,), report or None) cut at the k
        circles found; an EkfError carries .known, .centres, .assoc, .best and that rule's .report as they stood."""
        r = self._scan(ranges)
        max_readings = int(max_readings)
        if not 1 <= max_readings <= most:
            raise ValueError(f"1 <= max_readings <= {most}")
        k, cnt = C.c_int(int(known)), C.c_int(0)
        cen = np.zeros((max_readings, 2), dtype=np.float64)
        assoc, best = np.full(max_readings, -2, dtype=np.int32), np.empty(max_readings, dtype=np.float64)
        gates, rep = self._jcbb_args(jcbb, max_readings, "reading of max_readings", params)
        flags = self._lm_flags(deferred, grow_live)
        tail = [C.byref(rep)] if rep is not None else []

        def cut():
            return tuple(a[:cnt.value].copy() for a in (cen, assoc, best))
        try:
            _check(getattr(self._lib, call)(
                self._h, C.byref(params) if params is not None else None, r.ctypes.data_as(_dp), r.shape[0], max_readings,
                int(n_max), C.byref(k), *gates, flags, C.byref(cnt), cen.ctypes.data_as(_dp), assoc.ctypes.data_as(_ip),
                best.ctypes.data_as(_dp), *tail, None))
        except EkfError as e:
            e.known = k.value
            e.centres, e.assoc, e.best = cut()
            if rep is not None:
                e.report = rep.as_dict()
            raise
        return (k.value,) + cut() + (rep,)

    def associate_landmarks(self, readings, known, n_max, deferred=False, grow_live=False, params=None, joseph=False):
        """data_association (ekf_slam.cpp:278-402) for the readings (J, 2) in order, on the handle's own state: per reading
        the known landmarks are scored, the reference's rule is applied on the device, a new landmark is initialised
        (init_block's path, s = 0, W = sigma0 I), the winner is corrected (correct_sparse, or correct_sparse_deferred with
        deferred=True, correct_sparse_joseph with joseph=True) and the heading wrapped.  grow_live: a new landmark first
        grows the live dimension when it has to.
        Returns (known, assoc (J,) int32: landmark corrected / -1 dropped, best (J,), elapsed_ms).  A refused call or a
        singular S raises EkfError; the exception carries .known, .assoc and .best as they stood."""
        z = np.ascontiguousarray(readings, dtype=np.float64)
        if z.ndim != 2 or z.shape[1] != 2 or z.shape[0] < 1:
            raise ValueError("readings must be J x 2 with J >= 1")
        k, assoc, best, _, _, ms = self._associate_readings("ekf_dense64_associate_landmarks", z, known, n_max,
                                                            deferred, grow_live, params, joseph, groups=False)
        return k, assoc, best, ms

    @staticmethod
    def _scan(ranges):
        r = np.ascontiguousarray(ranges, dtype=np.float64)
        if r.ndim != 1 or not 1 <= r.shape[0] <= DensePropagator64.SCAN_MAX_BEAMS:
            raise ValueError(f"ranges must be one scan of 1 .. {DensePropagator64.SCAN_MAX_BEAMS} beams")
        return r

    def fit_scan(self, ranges, max_out=64, want_all=False):
        """CircleFitting::approxCirclePositions (circle_fitting.cpp:11-304) of ONE scan on the handle's device and stream: one
        workgroup, a wave per cluster; read-only with respect to the filter.  Returns (centres (k, 2), radii (k,),
        elapsed_ms), the first max_out circles in cluster order, and with want_all (centres, radii, all (c, 4) = x, y, r,
        is_circle of every cluster, elapsed_ms)."""
        r = self._scan(ranges)
        max_out = int(max_out)
        if not 1 <= max_out <= self.SCAN_MAX_CIRCLES:
            raise ValueError(f"1 <= max_out <= {self.SCAN_MAX_CIRCLES}")
        cen, rad = np.empty((max_out, 2), dtype=np.float64), np.empty(max_out, dtype=np.float64)
        allc = np.empty((self.SCAN_MAX_CIRCLES, 4), dtype=np.float64) if want_all else None
        cnt, ncl, ms = C.c_int(), C.c_int(), C.c_double()
        _check(self._lib.ekf_dense64_fit_scan(self._h, r.ctypes.data_as(_dp), r.shape[0], max_out, C.byref(cnt),
                                              cen.ctypes.data_as(_dp), rad.ctypes.data_as(_dp),
                                              allc.ctypes.data_as(_dp) if want_all else None, C.byref(ncl), C.byref(ms)))
        if want_all:
            return cen[:cnt.value].copy(), rad[:cnt.value].copy(), allc[:ncl.value].copy(), ms.value
        return cen[:cnt.value].copy(), rad[:cnt.value].copy(), ms.value

    def associate_scan(self, ranges, known, n_max, max_readings=64, deferred=False, grow_live=False, params=None):
        """fit_scan(ranges, max_readings) followed by associate_landmarks' per-reading path on the circles it finds, in
        cluster order, in one call: the landmarks node and the unknown_data_assoc node of the reference.  Returns (known,
        centres (k, 2), assoc (k,) int32, best (k,)); a scan without a circle gives k = 0 and writes nothing.  A refused call
        or a singular S raises EkfError; the exception carries .known, .centres, .assoc and .best as they stood."""
        return self._associate_scan("ekf_dense64_associate_scan", ranges, max_readings, self.SCAN_MAX_CIRCLES, known,
                                    n_max, deferred, grow_live, params)[:4]

    @staticmethod
    def _readings(readings, most):
        z = np.ascontiguousarray(readings, dtype=np.float64)
        if z.ndim != 2 or z.shape[1] != 2 or not 1 <= z.shape[0] <= most:
            raise ValueError(f"readings must be J x 2 with 1 <= J <= {most}")
        return z

    def score_readings(self, readings, first_lm=0, count=None, params=None):
        """score_landmarks() for the readings (J, 2) of a whole scan at once: candidate (j, i) is reading j against landmark
        first_lm + i, its nis and flag bit for bit those of score_landmarks for reading j alone.  The readings go up in one
        copy, the launches are cut at 32768 / count readings, one synchronisation; read-only.  Returns (nis (J, count),
        flags (J, count), elapsed_ms)."""
        z = self._readings(readings, self.JOINT_MAX_READINGS)
        first_lm = int(first_lm)
        if count is None:
            count = (self.live - 3) // 2 - first_lm
        count = int(count)
        if first_lm < 0 or not 1 <= count <= self.SCORE_SPARSE_MAX_ROWS // 2:
            raise ValueError(f"first_lm >= 0 and 1 <= count <= {self.SCORE_SPARSE_MAX_ROWS // 2}")
        J = z.shape[0]
        nis, flags = np.empty((J, count), dtype=np.float64), np.empty((J, count), dtype=np.int32)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_score_readings(
            self._h, C.byref(params) if params is not None else None, J, z.ctypes.data_as(_dp), first_lm, count,
            nis.ctypes.data_as(_dp), flags.ctypes.data_as(_ip), C.byref(ms)))
        return nis, flags, ms.value

    def joint_operands(self, lm_idx, readings, params=None):
        """The stacked operands the joint correction would use for the V pairs (landmark lm_idx[v], reading v), built on the
        device from the current state; read-only.  Returns (cols (3 + 2V,), Hc (2V, 3 + 2V), nu (2V,) bearing wrapped,
        elapsed_ms); R = r_meas I is implied.  Handed to correct_sparse[_deferred] they are one group of associate_joint."""
        z = self._readings(readings, self.JOINT_MAX_PAIRS)
        lm = np.ascontiguousarray(lm_idx, dtype=np.int32)
        V = z.shape[0]
        if lm.shape != (V,):
            raise ValueError("lm_idx must hold one landmark per reading")
        cols = np.empty(3 + 2 * V, dtype=np.int32)
        Hc, nu = np.empty((2 * V, 3 + 2 * V), dtype=np.float64), np.empty(2 * V, dtype=np.float64)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_joint_operands(
            self._h, C.byref(params) if params is not None else None, V, lm.ctypes.data_as(_ip), z.ctypes.data_as(_dp),
            cols.ctypes.data_as(_ip), Hc.ctypes.data_as(_dp), nu.ctypes.data_as(_dp), C.byref(ms)))
        return cols, Hc, nu, ms.value

    def associate_joint(self, readings, known, n_max, deferred=False, grow_live=False, params=None):
        """A whole scan associated jointly: all readings (J, 2) are scored against the state on entry, ONE assignment is made
        (of the readings that claim one landmark the lowest score keeps it, the readings under no gate take new slots in
        order), the new landmarks are initialised in groups of 32 and the matched and new readings are corrected in stacked
        updates of up to 30 readings (correct_sparse, or correct_sparse_deferred with deferred=True).  Not the sequential
        rule of associate_landmarks -- with one reading the two are the same in bits.  Two readings of one unseen object
        give two landmarks; find_duplicates / merge_landmarks is the repair.  Returns (known, assoc (J,) int32: landmark
        corrected / -1 dropped, best (J,), n_groups, elapsed_ms).  A refused call or a singular S raises EkfError; the
        exception carries .known, .assoc and .best as they stood."""
        z = self._readings(readings, self.JOINT_MAX_READINGS)
        k, assoc, best, _, ng, ms = self._associate_readings("ekf_dense64_associate_joint", z, known, n_max, deferred,
                                                             grow_live, params)
        return k, assoc, best, ng, ms

    def associate_scan_joint(self, ranges, known, n_max, max_readings=64, deferred=False, grow_live=False, params=None):
        """fit_scan(ranges, max_readings) followed by associate_joint's path on the circles it finds, in one call.  Returns
        (known, centres (k, 2), assoc (k,) int32, best (k,)) as associate_scan does; the exception of a refused call or a
        singular S carries .known, .centres, .assoc and .best as they stood."""
        return self._associate_scan("ekf_dense64_associate_scan_joint", ranges, max_readings, self.SCAN_MAX_CIRCLES,
                                    known, n_max, deferred, grow_live, params)[:4]

    def jcbb_launch_info(self):
        """(tile, threads) of the cross-block kernel: a workgroup computes tile x tile blocks W[p][q], a thread each"""
        tile, threads = C.c_int(), C.c_int()
        _check(self._lib.ekf_dense64_jcbb_launch_info(self._h, C.byref(tile), C.byref(threads)))
        return tile.value, threads.value

    def _gate_ic(self, gate_ic, params):
        return float(gate_ic if gate_ic is not None else (params.gate_update if params is not None else 1.0))

    def jcbb_candidates(self, readings, known, gate_ic=None, max_cand=4, params=None):
        """The device half of the joint compatibility association, read-only (pending rows are applied first): per reading
        the up to max_cand lowest (score, landmark) pairs under gate_ic (None: gate_update) in ascending order, and the
        cross blocks between all P candidates.  Returns a dict: cand_count (J,), cand_lm (J, max_cand; -1 beyond the count),
        cand_nis (J, max_cand; inf beyond it), best (J,), is_new (J,), P, reading_of (P,), lm_of (P,), nis (P,), W (2P, 2P)
        whose diagonal blocks are score_landmarks()' S bit for bit, nu (P, 2) raw, elapsed_ms -- what jcbb_search() takes."""
        z = self._readings(readings, self.JCBB_MAX_READINGS)
        J, max_cand = z.shape[0], int(max_cand)
        if not 1 <= max_cand <= self.JCBB_MAX_CAND:
            raise ValueError(f"1 <= max_cand <= {self.JCBB_MAX_CAND}")
        cap = min(J * max_cand, self.JCBB_MAX_READINGS * self.JCBB_MAX_CAND)
        count, is_new = np.zeros(J, dtype=np.int32), np.zeros(J, dtype=np.int32)
        lm, nis = np.full((J, max_cand), -1, dtype=np.int32), np.full((J, max_cand), np.inf)
        best, W, nu = np.zeros(J), np.zeros(4 * cap * cap), np.zeros((cap, 2))
        P, ms = C.c_int(0), C.c_double()
        _check(self._lib.ekf_dense64_jcbb_candidates(
            self._h, C.byref(params) if params is not None else None, J, z.ctypes.data_as(_dp), int(known),
            self._gate_ic(gate_ic, params), max_cand, count.ctypes.data_as(_ip), lm.ctypes.data_as(_ip),
            nis.ctypes.data_as(_dp), best.ctypes.data_as(_dp), is_new.ctypes.data_as(_ip), C.byref(P), W.ctypes.data_as(_dp),
            nu.ctypes.data_as(_dp), C.byref(ms)))
        n = P.value
        pick = [(j, c) for j in range(J) for c in range(count[j])]
        return {"cand_count": count, "cand_lm": lm, "cand_nis": nis, "best": best, "is_new": is_new, "P": n,
                "reading_of": np.array([j for j, _ in pick], dtype=np.int32),
                "lm_of": np.array([lm[j, c] for j, c in pick], dtype=np.int32),
                "nis": np.array([nis[j, c] for j, c in pick], dtype=np.float64),
                "W": W[:4 * n * n].reshape(2 * n, 2 * n).copy(), "nu": nu[:n].copy(), "elapsed_ms": ms.value}

    @staticmethod
    def jcbb_search(J, reading_of, lm_of, nis, W, nu, gate_joint, max_nodes=1 << 16):
        """The host half: the bounded branch and bound of ekf_dense64_jcbb_search over candidates in (reading, rank) order.
        Needs no handle and no device.  gate_joint (J,): the gate of a hypothesis of k pairings at [k - 1].  Returns (assign
        (J,) int32: candidate number or -1, report dict: n_cand, n_pairs, n_new, n_drop, exhausted, nodes, d2)."""
        r = np.ascontiguousarray(reading_of, dtype=np.int32)
        l = np.ascontiguousarray(lm_of, dtype=np.int32)
        P = r.shape[0]
        s = np.ascontiguousarray(nis if nis is not None else np.zeros(P), dtype=np.float64)
        Wm = np.ascontiguousarray(W, dtype=np.float64)
        v = np.ascontiguousarray(nu, dtype=np.float64).reshape(-1)
        g = np.ascontiguousarray(gate_joint, dtype=np.float64)
        if l.shape != (P,) or s.shape != (P,) or Wm.size != 4 * P * P or v.shape != (2 * P,) or g.shape != (int(J),):
            raise ValueError("reading_of, lm_of, nis (P,), W (2P, 2P), nu (P, 2), gate_joint (J,)")
        assign, rep = np.full(int(J), -1, dtype=np.int32), JcbbReport()
        _check(load().ekf_dense64_jcbb_search(int(J), P, r.ctypes.data_as(_ip), l.ctypes.data_as(_ip), s.ctypes.data_as(_dp),
                                              Wm.ctypes.data_as(_dp), v.ctypes.data_as(_dp), g.ctypes.data_as(_dp),
                                              int(max_nodes), assign.ctypes.data_as(_ip), C.byref(rep)))
        return assign, rep.as_dict()

    def associate_jcbb(self, readings, known, n_max, gate_ic=None, gate_joint=None, max_nodes=1 << 16, deferred=False,
                       grow_live=False, params=None):
        """A whole scan associated by joint compatibility (JCBB): the largest set of pairings whose stacked innovation
        passes one gate against its joint covariance, found by a bounded search over the device's candidates and cross
        blocks; unpaired readings under no landmark's gate_new become new landmarks, the rest drop; initialisation and
        stacked corrections exactly as associate_joint().  gate_ic None: gate_update; gate_joint None: k * gate_ic.
        Returns (known, assoc (J,) int32, best (J,), report dict, n_groups, elapsed_ms); the exception of a refused call or
        a singular S carries .known, .assoc, .best and .report as they stood."""
        z = self._readings(readings, self.JCBB_MAX_READINGS)
        k, assoc, best, rep, ng, ms = self._associate_readings("ekf_dense64_associate_jcbb", z, known, n_max, deferred,
                                                               grow_live, params, jcbb=(gate_ic, gate_joint, max_nodes))
        return k, assoc, best, rep.as_dict(), ng, ms

    def associate_scan_jcbb(self, ranges, known, n_max, max_readings=32, gate_ic=None, gate_joint=None, max_nodes=1 << 16,
                            deferred=False, grow_live=False, params=None, want_report=False):
        """fit_scan(ranges, max_readings <= 32) followed by associate_jcbb's path on the circles it finds, in one call.
        Returns (known, centres (k, 2), assoc (k,) int32, best (k,)) as associate_scan does, with want_report also the
        report dict (all zero for a scan without a circle); the exception carries .report too."""
        out = self._associate_scan("ekf_dense64_associate_scan_jcbb", ranges, max_readings, self.JCBB_MAX_READINGS,
                                   known, n_max, deferred, grow_live, params, jcbb=(gate_ic, gate_joint, max_nodes))
        return out[:4] + (out[4].as_dict(),) if want_report else out[:4]

    def predict_landmarks(self, dtheta, dx, want_terms=False, params=None):
        """prediction() (ekf_slam.cpp:55-106) for the twist (dtheta, dx) on the handle's own state: Fr = I + A, Qr = q_pose I
        and the pose update are built on the device from state[0] (both branches of :79, |dtheta| < straight_eps is the
        straight one), then exactly what propagate_block(0, Fr, Qr, dx) launches -- carry, pending rows and the live
        dimension as there; the heading is not wrapped.  Nothing goes up, no state comes down.  Returns elapsed_ms, and
        with want_terms (elapsed_ms, Fr (3, 3), dx (3,)) -- handed to propagate_block on a twin they give the same bits."""
        Fr = np.empty((3, 3), dtype=np.float64) if want_terms else None
        upd = np.empty(3, dtype=np.float64) if want_terms else None
        ms = C.c_double()
        _check(self._lib.ekf_dense64_predict_landmarks(
            self._h, C.byref(params) if params is not None else None, float(dtheta), float(dx),
            Fr.ctypes.data_as(_dp) if want_terms else None, upd.ctypes.data_as(_dp) if want_terms else None, C.byref(ms)))
        return (ms.value, Fr, upd) if want_terms else ms.value

    def measure_landmarks(self, sensor_xy, visible, initialised, deferred=False, want_terms=False, params=None,
                          joseph=False):
        """measurement() (ekf_slam.cpp:108-197) on the handle's own state: sensor_xy (n_lm, 2) holds a reading per
        landmark, visible (n_lm,) says which are corrected, initialised is the reference's landmark_init_flag.  The pose
        is captured once per call on the device and every correction of the call uses it; with initialised false ALL
        n_lm landmarks are first placed from their readings (Sigma untouched).  Then per visible landmark, ascending:
        correct_sparse (correct_sparse_deferred with deferred=True, correct_sparse_joseph with joseph=True) on
        device-built operands and the heading wrap.
        Returns (initialised, corrected, elapsed_ms), and with want_terms also (Hc (V, 2, 5), nu (V, 2) wrapped).  A
        singular S raises EkfError (EKF_ERR_STATE); the exception carries .initialised and .corrected as they stood."""
        z = np.ascontiguousarray(sensor_xy, dtype=np.float64)
        if z.ndim == 1 and z.size % 2 == 0:
            z = z.reshape(-1, 2)
        if z.ndim != 2 or z.shape[1] != 2 or z.shape[0] < 1:
            raise ValueError("sensor_xy must be n_lm x 2 with n_lm >= 1")
        n_lm = z.shape[0]
        vis = np.ascontiguousarray(np.asarray(visible) != 0, dtype=np.uint8)
        if vis.shape != (n_lm,):
            raise ValueError("visible must have length n_lm")
        V = int(vis.sum())
        Hc = np.empty((V, 2, 5), dtype=np.float64) if want_terms else None
        nu = np.empty((V, 2), dtype=np.float64) if want_terms else None
        flag, done, ms = C.c_int(1 if initialised else 0), C.c_int(0), C.c_double()
        flags = self._lm_flags(deferred, joseph=joseph)
        try:
            _check(self._lib.ekf_dense64_measure_landmarks(
                self._h, C.byref(params) if params is not None else None, n_lm, z.ctypes.data_as(_dp),
                vis.ctypes.data_as(_bp), C.byref(flag), flags, C.byref(done),
                Hc.ctypes.data_as(_dp) if want_terms else None, nu.ctypes.data_as(_dp) if want_terms else None,
                C.byref(ms)))
        except EkfError as e:
            e.initialised, e.corrected = bool(flag.value), done.value
            raise
        if want_terms:
            return bool(flag.value), done.value, ms.value, (Hc, nu)
        return bool(flag.value), done.value, ms.value

    def init_block(self, first, G=None, cols=None, W=None, xb=None, r=None):
        """(Re)initialise the states b = [first, first + r) as a function of the s states in cols: Sigma <- F Sigma F^T + Q
        for F = identity with F[b, b] = 0, F[b, cols] = G and Q = zero with Q[b, b] = W; state[b] = xb.  G: r x s with cols
        (s distinct indices in [0, N), none inside b), or both None (s = 0: the block's rows and columns become +0, its
        corner W, Sigma is not read -- with W = 100 I the prior of the reference's constructor, ekf_slam.cpp:27-36);
        W: r x r or None (no addition); xb: r or None (state untouched); r: taken from G, W or xb when not given.  Only
        the block's rows and columns of Sigma are written; the corner is bit for bit the S of
        score_sparse(cols[None], G[None], W) taken before the call.  Returns elapsed_ms."""
        if (G is None) != (cols is None):
            raise ValueError("G and cols come together (both None: s = 0)")
        if G is not None:
            G = np.ascontiguousarray(G, dtype=np.float64)
            if G.ndim != 2:
                raise ValueError("G must be r x s")
        if W is not None:
            W = np.ascontiguousarray(W, dtype=np.float64)
            if W.ndim != 2 or W.shape[0] != W.shape[1]:
                raise ValueError("W must be r x r")
        if xb is not None:
            xb = np.ascontiguousarray(xb, dtype=np.float64)
            if xb.ndim != 1:
                raise ValueError("xb must have length r")
        sizes = [int(r)] if r is not None else []
        sizes += [a.shape[0] for a in (G, W, xb) if a is not None]
        if not sizes or any(v != sizes[0] for v in sizes):
            raise ValueError("r must be given by r, G, W or xb, and all of them must agree")
        r = sizes[0]
        if not 1 <= r <= min(self.N, self.MAX_R):
            raise ValueError(f"1 <= r <= min(N, {self.MAX_R})")
        first = int(first)
        if not 0 <= first <= self.N - r:
            raise ValueError("the block [first, first + r) must lie inside [0, N)")
        s, pc, pg = 0, None, None
        if cols is not None:
            a = np.asarray(cols)
            if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
                raise ValueError("cols must be a one-dimensional integer array, not empty (s = 0: cols = G = None)")
            s = a.shape[0]
            if s > min(self.N - r, self.MAX_S):
                raise ValueError(f"cols must list s columns with s <= min(N - r, {self.MAX_S})")
            if a.min() < 0 or a.max() >= self.N:
                raise ValueError("every index in cols must lie in [0, N)")
            if len(np.unique(a)) != s:
                raise ValueError("no index may appear twice in cols")
            if ((a >= first) & (a < first + r)).any():
                raise ValueError("no index of cols may lie inside [first, first + r): that case is propagate_block")
            if G.shape != (r, s):
                raise ValueError("G must be r x s")
            cols = np.ascontiguousarray(a, dtype=np.int32)
            pc, pg = cols.ctypes.data_as(_ip), G.ctypes.data_as(_dp)
        ms = C.c_double()
        _check(self._lib.ekf_dense64_init_block(self._h, first, r, s, pc, pg,
                                                W.ctypes.data_as(_dp) if W is not None else None,
                                                xb.ctypes.data_as(_dp) if xb is not None else None, C.byref(ms)))
        return ms.value

    def swap_blocks(self, first_a, first_b, r):
        """Exchange the states [first_a, first_a + r) and [first_b, first_b + r): Sigma <- P Sigma P^T, state <- P state,
        a pure copy of 2 r rows and 2 r columns in which every entry keeps its bits.  The blocks are disjoint (adjacent is
        allowed) and lie inside the live dimension; either order gives the same result.  With carry on and rows pending
        the pending rows take the same permutation and nothing is flushed; otherwise it flushes first.  Removing a landmark
        in mid-map: swap_blocks(first, last, 2); init_block(last, W=prior); live -= 2.  Returns elapsed_ms."""
        first_a, first_b, r = int(first_a), int(first_b), int(r)
        if not 1 <= r <= min(self.N, self.MAX_R):
            raise ValueError(f"1 <= r <= min(N, {self.MAX_R})")
        if not (0 <= first_a <= self.N - r and 0 <= first_b <= self.N - r):
            raise ValueError("both blocks must lie inside [0, N)")
        if abs(first_a - first_b) < r:
            raise ValueError("the blocks must be disjoint: |first_a - first_b| >= r")
        ms = C.c_double()
        _check(self._lib.ekf_dense64_swap_blocks(self._h, first_a, first_b, r, C.byref(ms)))
        return ms.value

    def _read_list(self, idx, name):
        a = np.asarray(idx)
        if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"{name} must be a one-dimensional integer array, not empty")
        if a.min() < 0 or a.max() >= self.N:
            raise ValueError(f"every index in {name} must lie in [0, N)")
        return np.ascontiguousarray(a, dtype=np.int32)

    def sigma_block(self, rows, cols):
        """Sigma[np.ix_(rows, cols)] without reading Sigma back: one small gather on the device and one copy.  Indices
        in [0, N), repeats and any order allowed, len(rows) * len(cols) <= READ_MAX."""
        rows, cols = self._read_list(rows, "rows"), self._read_list(cols, "cols")
        if len(rows) * len(cols) > self.READ_MAX:
            raise ValueError(f"len(rows) * len(cols) must not exceed {self.READ_MAX}")
        out = np.empty((len(rows), len(cols)), dtype=np.float64)
        _check(self._lib.ekf_dense64_get_sigma_block(self._h, len(rows), rows.ctypes.data_as(_ip), len(cols),
                                                     cols.ctypes.data_as(_ip), out.ctypes.data_as(_dp)))
        return out

    def _state_range(self, first, count):
        first, count = int(first), int(count)
        if count < 1 or first < 0 or first + count > self.N:
            raise ValueError("the slice [first, first + count) must be non-empty and lie inside [0, N)")
        return first, count

    def state_block(self, first, count):
        """state[first:first + count] without moving the whole vector"""
        first, count = self._state_range(first, count)
        out = np.empty(count, dtype=np.float64)
        _check(self._lib.ekf_dense64_get_state_block(self._h, first, count, out.ctypes.data_as(_dp)))
        return out

    def set_state_block(self, first, x):
        """state[first:first + len(x)] = x; the rest of the state is not touched"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        if x.ndim != 1:
            raise ValueError("x must be one-dimensional")
        first, count = self._state_range(first, x.shape[0])
        _check(self._lib.ekf_dense64_set_state_block(self._h, first, count, x.ctypes.data_as(_dp)))

    def launch_info(self):
        """{ld, tiles, n_big, n_tail}: how one product is cut into 128 x 128 tiles and a quarter-tile tail (test hook)"""
        return self._launch_info()


class _Region:
    """DensePropagator64.region(Na)"""

    def __init__(self, handle, Na):
        self._d, self._Na, self.report = handle, int(Na), None

    def __enter__(self):
        self._d.region_begin(self._Na)
        return self

    def __exit__(self, *exc):
        if self._d.region_info()["active"]:
            self.report = self._d.region_end()
        return False


class DenseEKFSLAM:
    """rigid2d::EKF_SLAM (ekf_slam.hpp:19-57) on one DensePropagator64 handle: the reference's three methods, each one call
    into the library, the state never leaving the device.  n landmarks in a handle with room for `capacity` (default n).
    deferred: the corrections go through the pending rows; carry: prediction() and a new landmark leave them pending;
    grow_live: the live dimension starts at the pose and data_association() grows it as the map is discovered
    (measurement() places all n landmarks, so it raises it to 3 + 2 n); joseph: the corrections of measurement(),
    data_association() and merge() run in the Joseph form (eager only).  `handle` is the DensePropagator64 underneath."""

    PRIOR = 100.0   # the reference's landmark prior (ekf_slam.cpp:32)

    def __init__(self, n, capacity=None, deferred=False, carry=False, grow_live=False, params=None, device=-1,
                 joseph=False):
        self.n = int(n)
        cap = self.n if capacity is None else int(capacity)
        if self.n < 1 or cap < self.n:
            raise ValueError("n >= 1 and capacity >= n")
        if deferred and joseph:
            raise ValueError("joseph is an eager form: not with deferred")
        self.deferred, self.grow_live, self.params, self.joseph = bool(deferred), bool(grow_live), params, bool(joseph)
        self._device = device
        self.handle = d = DensePropagator64(3 + 2 * cap, device)
        # the constructor's prior (:27-46): Sigma zero (as created) except 100 I on the landmarks; the state zero
        for first in range(3, d.N, d.MAX_R):
            r = min(d.MAX_R, d.N - first)
            d.init_block(first, W=self.PRIOR * np.eye(r))
        d.carry = bool(carry)
        d.live = 3 if self.grow_live else 3 + 2 * self.n
        self._known, self._init_flag = 0, False
        self.jcbb_report = None   # the report of the last jcbb_association() / scan_association(joint="jcbb")
        self._logodds = np.zeros(0, dtype=np.float64)   # scan_evidence()'s verdicts so far, one per mapped landmark
        self.evidence = None      # the ScanEvidence of the last scan_evidence() / scan_association(evidence=True)

    def close(self):
        self.handle.close()

    def prediction(self, dtheta, dx):
        """prediction(Twist2D(dtheta, dx, 0)); returns elapsed_ms"""
        return self.handle.predict_landmarks(dtheta, dx, params=self.params)

    def measurement(self, sensor_xy, visible):
        """measurement(sensor_reading, visible_list, .); returns the number of corrections"""
        d = self.handle
        if d.live < 3 + 2 * self.n:
            d.live = 3 + 2 * self.n
        try:
            self._init_flag, done, _ = d.measure_landmarks(sensor_xy, visible, self._init_flag, self.deferred,
                                                           params=self.params, joseph=self.joseph)
        except EkfError as e:
            self._init_flag = e.initialised
            raise
        return done

    def data_association(self, meas_xy):
        """data_association(measures, known_list) with the known list kept by the object; returns assoc (J,) int32: the
        landmark each reading corrected, -1 for a dropped one"""
        try:
            self._known, assoc, _, _ = self.handle.associate_landmarks(meas_xy, self._known, self.n, self.deferred,
                                                                       self.grow_live, self.params, self.joseph)
        except EkfError as e:
            self._known = e.known
            raise
        return assoc

    def joint_association(self, meas_xy):
        """the readings of one scan associated jointly (DensePropagator64.associate_joint): all scored against the state on
        entry, one assignment, stacked corrections; returns assoc (J,) int32 as data_association() does"""
        try:
            self._known, assoc, _, _, _ = self.handle.associate_joint(meas_xy, self._known, self.n, self.deferred,
                                                                      self.grow_live, self.params)
        except EkfError as e:
            self._known = e.known
            raise
        return assoc

    def jcbb_association(self, meas_xy, gate_ic=None, gate_joint=None, max_nodes=1 << 16):
        """the readings of one scan associated by joint compatibility (DensePropagator64.associate_jcbb): the largest
        jointly compatible set of pairings, then joint_association()'s initialisation and stacked corrections; returns
        assoc (J,) int32 as data_association() does.  The report of the last call is .jcbb_report."""
        try:
            self._known, assoc, _, self.jcbb_report, _, _ = self.handle.associate_jcbb(
                meas_xy, self._known, self.n, gate_ic, gate_joint, max_nodes, self.deferred, self.grow_live, self.params)
        except EkfError as e:
            self._known = e.known
            raise
        return assoc

    def scan_association(self, ranges, joint=False, evidence=False, lidar=None):
        """one LaserScan through the landmarks node (circle fitting) into data_association() -- or, with joint=True, into
        joint_association(), with joint="jcbb" into jcbb_association() (at most 32 circles, the default gates) -- in one
        call; returns (centres (k, 2), assoc (k,) int32) of the k circles found.  evidence=True: scan_evidence(ranges,
        lidar) with its defaults runs behind the association, on the corrected map (lidar: the sensor's LidarParams,
        default_lidar() -- with its square wall -- if None; evidence=False: today's launches and nothing else)"""
        out = self._scan_association(ranges, joint)
        if evidence:
            self.scan_evidence(ranges, lidar)
        return out

    def _scan_association(self, ranges, joint):
        if isinstance(joint, str):
            if joint != "jcbb":
                raise ValueError('joint must be False, True or "jcbb"')
            try:
                self._known, centres, assoc, _, self.jcbb_report = self.handle.associate_scan_jcbb(
                    ranges, self._known, self.n, deferred=self.deferred, grow_live=self.grow_live, params=self.params,
                    want_report=True)
            except EkfError as e:
                self._known = e.known
                raise
            return centres, assoc
        call = self.handle.associate_scan_joint if joint else self.handle.associate_scan
        try:
            self._known, centres, assoc, _ = call(ranges, self._known, self.n, deferred=self.deferred,
                                                  grow_live=self.grow_live, params=self.params)
        except EkfError as e:
            self._known = e.known
            raise
        return centres, assoc

    def local_region(self, n_local):
        """context manager: a local region over the pose and the first n_local landmarks (3 + 2 n_local states).  While it
        is open prediction() and the handle's structured calls on those landmarks (handle.correct_sparse(),
        handle.score_landmarks(), handle.measure_landmarks() with n_lm = n_local, ...) cost what a map of n_local
        landmarks costs, and the rest of the map is paid once at the end -- exact for a surveyed (coupled) map.
        measurement() addresses all n landmarks and therefore ends the region; data_association() is refused while
        known landmarks lie beyond it.  The caller brings
        the landmarks it sees into the prefix with handle.swap_blocks() first."""
        return self.handle.region(3 + 2 * int(n_local))

    def find_duplicates(self, gate, r_merge):
        """the pairs (a, b), a < b, of known landmarks that are each other's nearest partner with d2 < gate, in ascending
        a, from one landmark_pairs() scan -> (pairs [(a, b, d2)], n_below)"""
        if self._known < 2:
            return [], 0
        nearest, d2, below, _, _ = self.handle.landmark_pairs(self._known, r_merge, gate)
        pairs = [(a, int(b), float(d2[a])) for a, b in enumerate(nearest) if b > a and nearest[b] == a and d2[a] < gate]
        return pairs, below

    def merge(self, a, b, r_merge):
        """fuse the known landmarks a and b and remove the higher (merge_landmarks on the object's paths); the last known
        landmark moves into its slot.  Returns (moved_from, d2)"""
        flags = self.handle._lm_flags(self.deferred, self.grow_live, self.joseph)
        l = self.logodds
        self._known, moved, d2, _ = self.handle.merge_landmarks(a, b, r_merge, self._known, flags, self.params)
        self._logodds_removed(l, max(int(a), int(b)), moved)
        return moved, d2

    # ---- scan evidence: which landmark is spurious -----------------------------------------------------------------------
    @property
    def logodds(self):
        """(mapped landmarks,) float64: the log-odds scan_evidence() keeps per landmark, 0 for one it has not judged yet.
        The array is the object's own and follows the landmarks through merge(), remove(), prune(), join(), clone() and
        submap()."""
        k = self._mapped()
        if self._logodds.shape[0] != k:
            grown = np.zeros(k, dtype=np.float64)
            m = min(k, self._logodds.shape[0])
            grown[:m] = self._logodds[:m]
            self._logodds = grown
        return self._logodds

    def _logodds_removed(self, l, slot, moved):
        """the bookkeeping of a removal: the landmark `moved` (the old last one, -1: none) sits in `slot`, the last is gone"""
        if moved >= 0:
            l[slot] = l[moved]
        self._logodds = l[:-1].copy()

    def scan_evidence(self, ranges, lidar=None, tol_abs=0.05, kappa=2.0, min_beams=3, w_hit=0.4, w_miss=0.85,
                      l_min=-4.0, l_max=4.0):
        """one LaserScan cast against the map (DensePropagator64.scan_evidence over the mapped landmarks) and its verdicts
        added to .logodds (evidence_update): a landmark most of whose beams stop on it gains w_hit, one most of whose
        beams go through the place where it should stand loses w_miss.  Read-only on the filter.  Returns verdict
        (mapped,) int32: +1, -1 or 0; the counts are in .evidence."""
        k = self._mapped()
        if k < 1:
            self.evidence = None
            return np.zeros(0, dtype=np.int32)
        self.evidence = ev = self.handle.scan_evidence(ranges, lidar, 0, k, tol_abs, kappa, self.params)
        return evidence_update(self.logodds, ev.n_expected, ev.n_agree, ev.n_through, min_beams, w_hit, w_miss, l_min, l_max)

    def add_landmark(self, xy, W=None):
        """a landmark the caller knows of by other means (a surveyed tube, a map from an earlier run) becomes the next known
        landmark: init_block(s = 0) puts it at xy in the state's frame with the covariance block W (2 x 2, default the
        landmark prior), uncorrelated with everything else.  Its log-odds start at 0.  Returns its index."""
        if self._init_flag:
            raise ValueError("add_landmark() appends behind the known landmarks of data_association(); measurement() placed all n")
        if self._known >= self.n:
            raise ValueError(f"the map is full: n = {self.n}")
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1)
        if xy.shape != (2,):
            raise ValueError("xy must be one position")
        prior = (self.params if self.params is not None else default_params()).sigma0_landmark
        W = prior * np.eye(2) if W is None else np.ascontiguousarray(W, dtype=np.float64)
        d, i = self.handle, self._known
        if d.live < 3 + 2 * (i + 1):
            d.live = 3 + 2 * (i + 1)
        d.init_block(3 + 2 * i, W=W, xb=xy)
        self._known = i + 1
        return i

    def remove(self, i):
        """remove the known landmark i (DensePropagator64.remove_landmark on the object's paths); the last known landmark
        moves into its slot, and its log-odds with it.  Returns moved_from (-1: i was the last)"""
        if self._init_flag:
            raise ValueError("remove() drops a known landmark of data_association(); measurement() placed all n")
        l = self.logodds
        flags = self.handle.LM_GROW_LIVE if self.grow_live else 0
        self._known, moved, _ = self.handle.remove_landmark(i, self._known, flags, self.params)
        self._logodds_removed(l, int(i), moved)
        return moved

    def prune(self, threshold):
        """remove every known landmark whose log-odds are < threshold, highest index first (so the landmark that moves
        into a freed slot has been judged already); returns the indices removed, as they were before the call"""
        doomed = [int(i) for i in np.nonzero(self.logodds < threshold)[0][::-1]]
        for i in doomed:
            self.remove(i)
        return doomed

    def health(self):
        """DensePropagator64.health() of the live corner: is the covariance still one?"""
        return self.handle.health()

    def symmetrize(self):
        """DensePropagator64.symmetrize(): both halves of the live corner equal again, at the caller's cadence"""
        return self.handle.symmetrize()

    def _mapped(self):
        return self.n if self._init_flag else self._known

    def observation_value(self, range_max=None):
        """DensePropagator64.rank_landmarks() over the landmarks the map has (all n after measurement(), the known ones of
        data_association() otherwise): what looking at each of them next would take off tr Sigma, off the pose variances
        and off the entropy.  range_max: the sensor's reach, None = unlimited."""
        k = self._mapped()
        if k < 1:
            raise ValueError("the map has no landmark yet")
        return self.handle.rank_landmarks(0, k, range_max, self.params)

    def best_view(self, k, by="trace", range_max=None):
        """the k landmarks most worth observing next, best first: by="trace" (drop of tr Sigma), "pose" (drop of the pose
        variances) or "info" (drop of the entropy); the lower index first among equal values.  -> int array (<= k)"""
        return self.observation_value(range_max).order(by)[:int(k)]

    def factor(self):
        """DensePropagator64.factor() of the live corner: definiteness and log det Sigma"""
        return self.handle.factor()

    def _framed(self, call):
        """run a frame change on the states the map has: all n landmarks after measurement(), the known ones of
        data_association() otherwise.  Below the live dimension the rest must be decoupled from them."""
        d = self.handle
        live = d.live
        W = 3 + 2 * (self.n if self._init_flag else self._known)
        if W > live:
            raise ValueError("the map reaches beyond the live dimension")
        if W < live:
            if d.coupling(W)[0] != 0:
                raise ValueError(f"states beyond {W} are coupled to the map: a frame change of the first {W} alone is not exact")
            d.live = W
        try:
            return call()
        finally:
            if W < live:
                d.live = live

    def reframe(self, dtheta, tx, ty):
        """the map and its covariance in the frame reached by the rigid transform q -> R(dtheta) q + (tx, ty)
        (DensePropagator64.reframe, FRAME_FIXED): what map_nees() needs when the truth comes in a world frame"""
        return self._framed(lambda: self.handle.reframe(DensePropagator64.FRAME_FIXED, dtheta, tx, ty))

    def robot_frame(self):
        """the map in the robot's own frame (FRAME_ROBOT); call it again before filtering on"""
        return self._framed(lambda: self.handle.reframe(DensePropagator64.FRAME_ROBOT))

    def join(self, other):
        """map joining (DensePropagator64.join_map): `other` is a DenseEKFSLAM that built a local map in the frame of this
        filter's robot pose, started at pose 0 and independent of this map.  Its known landmarks become this filter's
        landmarks known .. known + other.known - 1, the pose becomes the composition of the two; find_duplicates() and
        merge() then fuse what both maps saw.  States of either filter beyond its known landmarks must be decoupled from
        them, as for reframe() (coupling() is checked on both).  Two things beyond the library call: both live dimensions
        are set to 3 + 2 known for the call and put back afterwards -- on `other` too, which like the join itself flushes
        its pending rows; its state, its covariance values and, on return, its live dimension are as they were (reset or
        close it) -- and the call is refused once measurement() has placed all n landmarks of either filter, since
        there is then no "behind the known landmarks" to append to.  Returns elapsed_ms"""
        if not isinstance(other, DenseEKFSLAM):
            raise ValueError("join() takes another DenseEKFSLAM")
        if self._init_flag or other._init_flag:
            raise ValueError("join() appends behind the known landmarks of data_association(); measurement() placed all n")
        d, src = self.handle, other.handle
        if self._known + other._known > self.n:
            raise ValueError(f"{self._known} + {other._known} landmarks do not fit n = {self.n}")
        live, W = d.live, 3 + 2 * self._known
        src_live, Wb = src.live, 3 + 2 * other._known
        self.logodds   # (sized for the known landmarks before the other map's are appended)
        if W > live or Wb > src_live:
            raise ValueError("the map reaches beyond the live dimension")
        for h, w, lv in ((d, W, live), (src, Wb, src_live)):
            if w < lv and h.coupling(w)[0] != 0:
                raise ValueError(f"states beyond {w} are coupled to the map: a join of the first {w} alone is not exact")
        if W < live:
            d.live = W
        if Wb < src_live:
            src.live = Wb
        try:
            ms = d.join_map(src)
        finally:
            if Wb < src_live:
                src.live = src_live
            if d.live < live:
                d.live = live
        self._logodds = np.concatenate([self._logodds, other.logodds])
        self._known += other._known
        return ms

    def _copy_target(self, into):
        """the filter a copy goes into: a new one with this filter's n, capacity, flags and params, or `into` if it has them"""
        cap = (self.handle.N - 3) // 2
        if into is None:
            return DenseEKFSLAM(self.n, cap, self.deferred, self.handle.carry, self.grow_live, self.params, self._device,
                                self.joseph)
        if not isinstance(into, DenseEKFSLAM) or into is self:
            raise ValueError("`into` must be another DenseEKFSLAM")
        if (into.n, into.handle.N) != (self.n, self.handle.N):
            raise ValueError(f"`into` must have n = {self.n} and capacity = {cap}")
        if (into.deferred, into.grow_live, into.joseph) != (self.deferred, self.grow_live, self.joseph):
            raise ValueError("`into` must have the same deferred, grow_live and joseph flags")
        if into.handle.carry != self.handle.carry:
            raise ValueError("`into` must have the same carry flag")
        into.params = self.params
        return into

    def clone(self, into=None):
        """a second DenseEKFSLAM that holds the same filter (DensePropagator64.extract_map, one pass on the device, nothing
        through the host): the same n, capacity, flags and params, the same known landmarks, init flag, live dimension and
        -- in a deferred filter -- the same pending rows, which are carried and not applied, so a snapshot in mid-tick costs
        no flush.  The copy covers the live dimension; beyond it a new filter has the constructor's prior, as this one has,
        and a reused one keeps what it had (a grow_live filter initialises those states again when its map reaches them).
        into: a filter of the same shape and flags to overwrite instead of building one.  Snapshot, run data_association()
        on one and joint_association() on the other, keep one -- or restore()."""
        t = self._copy_target(into)
        t.handle.extract_map(self.handle)
        t._known, t._init_flag = self._known, self._init_flag
        t._logodds = self.logodds.copy()
        return t

    def restore(self, snap):
        """this filter becomes the one `snap` holds (a clone() taken earlier): snap.clone(into=self)"""
        if not isinstance(snap, DenseEKFSLAM):
            raise ValueError("restore() takes a DenseEKFSLAM")
        return snap.clone(into=self)

    def submap(self, keep, into=None):
        """a DenseEKFSLAM of the same shape that knows the landmarks keep[0], keep[1], ... of this filter (distinct, each in
        [0, known), any order) as its landmarks 0 .. k - 1, with this filter's pose: the marginal of the filter on them, which
        for an EKF is the deletion of the other rows and columns and therefore exact.  The inverse of join() (hand the
        submap to another process, join() it into a fresh global filter), and pruning in bulk (keep the k landmarks worth
        keeping, go on with the result).  Refused once measurement() has placed all n landmarks, as join() is.  Pending rows
        are carried.  A target that is not grow_live gets its live dimension back to 3 + 2 n, after coupling() has found
        the states beyond the submap decoupled from it (which flushes the carried rows): a new target has the
        constructor's prior there; a reused `into` may not, and is then refused -- with the submap in its first 3 + 2 k
        states and its live dimension there."""
        if self._init_flag:
            raise ValueError("submap() picks among the known landmarks of data_association(); measurement() placed all n")
        a = np.asarray(keep)
        if a.ndim != 1 or not (a.size == 0 or np.issubdtype(a.dtype, np.integer)):
            raise ValueError("keep must be a list of landmark indices (one dimension, integers)")
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= self._known):
            raise ValueError(f"every index of keep must be a known landmark, in [0, {self._known})")
        if np.unique(a).size != a.size:
            raise ValueError("keep names a landmark twice")
        t = self._copy_target(into)
        t.handle.extract_map(self.handle, a)
        t._known, t._init_flag = int(a.size), False
        t._logodds = self.logodds[a].copy()
        W, full = 3 + 2 * int(a.size), 3 + 2 * t.n
        if not t.grow_live and W < full:
            if t.handle.coupling(W)[0] != 0:
                raise ValueError(f"`into` holds states beyond {W} that are coupled to the submap (not the constructor's "
                                 f"prior): its live dimension stays {W}")
            t.handle.live = full
        return t

    def map_nees(self, truth):
        """(state - truth)^T Sigma^-1 (state - truth) over the live dimension against the last factor(): the NEES of the
        whole map, live degrees of freedom.  truth: the live states [theta, x, y, m1x, ...]; the heading difference is
        wrapped by the library's normalize_angles rule."""
        d = self.handle
        live = d.live
        truth = np.ascontiguousarray(truth, dtype=np.float64).reshape(-1)
        if truth.shape != (live,):
            raise ValueError("truth must hold the live states")
        e = d.state_block(0, live) - truth
        e[0] = normalize_angles(e[:1])[0]
        return float(d.whiten(e, want_Y=False)["d2"][0])

    def map_solve(self, e=None, truth=None):
        """Sigma^-1 e over the live dimension against the last factor(): half the gradient of map_nees with respect to the
        state.  Give the error vector e itself, or truth (the live states) for e = state - truth with the heading
        difference wrapped as map_nees wraps it."""
        d = self.handle
        live = d.live
        if (e is None) == (truth is None):
            raise ValueError("give e or truth")
        v = np.ascontiguousarray(truth if e is None else e, dtype=np.float64).reshape(-1)
        if v.shape != (live,):
            raise ValueError("e / truth must hold the live states")
        if e is None:
            v = d.state_block(0, live) - v
            v[0] = normalize_angles(v[:1])[0]
        return d.solve(v)["X"][0]

    def sample_maps(self, k, rng=None, Z=None):
        """k <= 64 maps drawn from N(state, Sigma of the last factor()), k x live: state + L z for rows z of unit normal
        draws -- Z (k x live) if given, rng.standard_normal((k, live)) otherwise (rng: a numpy Generator, default_rng() if
        None).  The state is the current one and the factor a snapshot: call factor() after the last correction.  The
        heading of a sample is not wrapped."""
        d = self.handle
        live = d.live
        if not 1 <= k <= d.WHITEN_MAX_RHS:
            raise ValueError(f"1 <= k <= {d.WHITEN_MAX_RHS}")
        if Z is None:
            Z = (np.random.default_rng() if rng is None else rng).standard_normal((k, live))
        Z = np.ascontiguousarray(Z, dtype=np.float64)
        if Z.shape != (k, live):
            raise ValueError("Z must be k x live")
        return d.color(Z, add_state=True)["X"]

    @property
    def state(self):
        """[theta, x, y, m1x, m1y, ...] of the n landmarks"""
        return self.handle.state_block(0, 3 + 2 * self.n)

    @property
    def pose(self):
        return self.handle.state_block(0, 3)

    @property
    def known(self):
        """landmarks data_association() has initialised: landmarks 0 .. known - 1"""
        return self._known

    @property
    def init_flag(self):
        """the reference's landmark_init_flag: measurement() has placed the landmarks"""
        return self._init_flag


MAX_CLUSTERS = 128


def simulate_scans(poses, world, seed=7, first_filter_id=0, step=0, lidar=None, device=-1):
    """poses [S, 3] = (theta, x, y) -> ranges [S, n_beams] from the on-device lidar simulator (host twin:
    synth.make_scans with fid = first_filter_id + s and the same step)."""
    lib = load()
    sp = SimParams()
    lib.ekf_default_sim_params(C.byref(sp))
    sp.seed, sp.first_filter_id = int(seed), int(first_filter_id)
    lp = lidar if lidar is not None else default_lidar()
    ps = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)
    w = np.ascontiguousarray(world, dtype=np.float64).reshape(-1, 2)
    out = np.empty((len(ps), lp.n_beams))
    _check(lib.ekf_simulate_scans(device, C.byref(sp), C.byref(lp), _d(w), len(w), _d(ps), len(ps), int(step), _d(out)))
    return out


def normalize_angles(values, device=-1):
    """rigid2d::normalize_angle (rigid2d.cpp:336-345) evaluated by the device helper the kernels use."""
    v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
    out = np.empty_like(v)
    _check(load().ekf_normalize_angles(device, _d(v), len(v), _d(out)))
    return out


def circle_fit_scans(ranges, max_out=32, device=-1, want_all=False):
    """Batched rigid2d::CircleFitting::approxCirclePositions (circle_fitting.cpp:298-304) on the GPU.
    ranges [S, n_beams] -> list of per-scan centre arrays [k_s, 2] and radii [k_s]
    (+ per-scan [c_s, 4] = x, y, r, is_circle of every cluster when want_all)."""
    r = np.ascontiguousarray(ranges, dtype=np.float64)
    if r.ndim == 1:
        r = r[None, :]
    S, nb = r.shape
    cen = np.zeros((S, max_out, 2))
    rad = np.zeros((S, max_out))
    cnt = np.zeros(S, dtype=np.int32)
    ncl = np.zeros(S, dtype=np.int32)
    allc = np.zeros((S, MAX_CLUSTERS, 4)) if want_all else None
    _check(load().ekf_circle_fit_scans(device, _d(r), S, nb, max_out, _d(cen), _d(rad), cnt.ctypes.data_as(_ip),
                                       _d(allc) if want_all else None, ncl.ctypes.data_as(_ip)))
    centres = [cen[s, :cnt[s]].copy() for s in range(S)]
    radii = [rad[s, :cnt[s]].copy() for s in range(S)]
    if want_all:
        return centres, radii, [allc[s, :ncl[s]].copy() for s in range(S)]
    return centres, radii
