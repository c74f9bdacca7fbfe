/*
 * ekfslam.h -- C ABI of libekfslam_hip.so, the MI355X (gfx950) EKF-SLAM filter core.
 *
 * Drop-in boundary for the hot path of tonylitianyu/EKF-SLAM-ML: the public class
 * rigid2d::EKF_SLAM (rigid2d/include/rigid2d/ekf_slam.hpp:19-57, implemented in
 * rigid2d/src/ekf_slam.cpp).  The reference has no FFI layer; the binding a maintainer
 * adds is a replacement for src/ekf_slam.cpp that forwards each method to one entry
 * point below (INTEGRATION.md shows it; host/ekf_slam.hpp is the header-only C++ mirror).
 *
 * Conventions
 *   - plain pointers and sizes only; caller-owned HOST buffers unless a name says _dev;
 *   - every function returns an ekf_status (0 = EKF_OK); no exceptions cross the boundary;
 *     ekf_last_error() gives the text of the calling thread's last failure;
 *   - one handle = one filter (or one batch of filters) bound to one HIP device and one HIP
 *     stream; a handle is NOT thread-safe (the reference is driven from ROS1's single-threaded
 *     spinner, nuslam/src/slam.cpp:525);
 *   - state order [theta, x, y, m1x, m1y, ...] (ekf_slam.cpp:15-21,72-74); N = 3 + 2n;
 *   - covariance crosses the boundary ROW-major N x N fp64; std::vector<bool> arguments of the
 *     reference cross as uint8_t[n] (0 / non-zero).
 *   - all arithmetic is fp64 like the reference (arma::mat = Mat<double>).
 */
#ifndef EKFSLAM_H
#define EKFSLAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    EKF_OK = 0,
    EKF_ERR_INVALID = 1,   /* bad argument (null pointer, n < 0, index out of range ...) */
    EKF_ERR_NO_DEVICE = 2, /* no HIP device / wrong architecture */
    EKF_ERR_HIP = 3,       /* a HIP runtime call failed, see ekf_last_error() */
    EKF_ERR_NOMEM = 4,     /* host or device allocation failed */
    EKF_ERR_STATE = 5      /* call sequence error (e.g. run before a log was uploaded) */
} ekf_status;

/* The reference hard-codes these; defaults reproduce it exactly. */
typedef struct {
    double sigma0_landmark; /* 100     ekf_slam.cpp:32      initial landmark variance       */
    double q_pose;          /* 1e-4    ekf_slam.cpp:40-43   process noise on theta, x, y    */
    double r_meas;          /* 0.01    ekf_slam.cpp:172-175 range / bearing noise           */
    double gate_new;        /* 10.0    ekf_slam.cpp:293     Mahalanobis gate: new landmark  */
    double gate_update;     /* 1.0     ekf_slam.cpp:330     Mahalanobis gate: apply update  */
    double straight_eps;    /* 1e-6    ekf_slam.cpp:79      |dtheta| below -> straight line */
} ekf_params;

typedef struct ekf_filter_s* ekf_handle;      /* one filter  == one rigid2d::EKF_SLAM object */
typedef struct ekf_batch_s* ekf_batch_handle; /* B independent filters (Monte-Carlo batch)   */

const char* ekf_last_error(void);
void ekf_default_params(ekf_params* out);
/* Doubles between the starts of two rows of a filter's covariance (and the length of its state / factor vectors) for a map of
 * n landmarks: N = 3 + 2 n rounded up to 16, or to 256 -- rows on 2-KB boundaries -- where that adds at most 1/32 of a row
 * (n = 1000: 2048).  A filter takes 8 N ld bytes of device memory for its covariance.  Needs no device. */
int ekf_leading_dimension(int n_landmarks);
/* Number of visible HIP devices (0 if none); does not initialise a device context. */
int ekf_device_count(void);

/* ---- single filter: the rigid2d::EKF_SLAM call surface ------------------------------------ */

/* EKF_SLAM::EKF_SLAM(int n_measurements)            ekf_slam.hpp:27, ekf_slam.cpp:27-53.
 * params may be NULL (reference constants).  device < 0 selects the current HIP device. */
ekf_status ekf_create(int n, const ekf_params* params, int device, ekf_handle* out);
ekf_status ekf_destroy(ekf_handle h);
/* Copy construction / copy assignment of the by-value member (nuslam/src/slam.cpp:213,428). */
ekf_status ekf_clone(ekf_handle h, ekf_handle* out);

/* void prediction(const Twist2D&)                   ekf_slam.hpp:31, ekf_slam.cpp:55-106.
 * dtheta = twist.angular(), dx = twist.linearX(); linearY is ignored by the reference (:70). */
ekf_status ekf_predict(ekf_handle h, double dtheta, double dx);

/* void measurement(mat sensor_reading, vector<bool> visible_list, vector<bool> known_list)
 *                                                   ekf_slam.hpp:36, ekf_slam.cpp:108-197.
 * sensor_xy: 2n doubles (robot-frame x,y per landmark = sensor_reading.memptr());
 * visible: n bytes.  known_list is unused by the reference and therefore not passed. */
ekf_status ekf_measure_known(ekf_handle h, const double* sensor_xy, const uint8_t* visible);

/* void data_association(vector<Vector2D> measures, vector<bool>& known_list)
 *                                                   ekf_slam.hpp:41, ekf_slam.cpp:278-402.
 * meas_xy: 2J doubles (Vector2D is {double x, y}, rigid2d.hpp:68-72, so &measures[0].x);
 * known: n bytes, IN/OUT (entries are set as landmarks are initialised, :323);
 * assoc_out: optional J ints, the landmark each measurement updated (-1 = dropped).
 * Synchronous in its RESULTS only: the call returns when the decisions and known_list are final; the gain of the last
 * reading and the call's pass over the covariance may still be running on the handle's stream.  An execution error of
 * that tail (or a device-side error word, EKF_ERR_HIP) therefore surfaces at the NEXT call that synchronises with the
 * stream (ekf_sync, any getter, the next ekf_associate); stream order keeps every later call behind it.
 * Which launch structure ("form") runs is chosen by map size; state, covariance, decisions and known_list are
 * bit-identical across forms.  Internal bookkeeping is not: the diagnostic winning distance of the association record
 * is only kept by the per-reading forms, and the touched set (ekf_set_active_set) is "every landmark below the known
 * count" on the call-fused forms and "landmarks actually corrected" on the others -- both supersets of what the
 * exact sparsity needs. */
ekf_status ekf_associate(ekf_handle h, const double* meas_xy, int J, uint8_t* known, int* assoc_out);

/* double calculate_maha_dis(Vector2D, int) for i in [0, M)   ekf_slam.hpp:86, ekf_slam.cpp:217-276.
 * Private in the reference; exposed as the parity hook of the one-landmark-per-wavefront
 * scoring kernel.  scores_out: M doubles. */
ekf_status ekf_maha_scores(ekf_handle h, double meas_x, double meas_y, int M, double* scores_out);

/* double rigid2d::normalize_angle(double)            rigid2d/src/rigid2d.cpp:336-345 (range (-pi, pi]).
 * Parity hook of the device helper every kernel uses: out[i] = normalize_angle(in[i]), count values. */
ekf_status ekf_normalize_angles(int device, const double* in, int count, double* out);

/* getStateTheta / getStateX / getStateY             ekf_slam.cpp:404-414 -> out = {theta, x, y} */
ekf_status ekf_get_pose(ekf_handle h, double out[3]);
/* mat getStateLandmark()                            ekf_slam.cpp:416-418 -> 2n doubles */
ekf_status ekf_get_landmarks(ekf_handle h, double* out);

/* snapshot / restore and test access to the private members state, sigma (ekf_slam.hpp:61-65) */
ekf_status ekf_dim(ekf_handle h, int* n, int* N);
ekf_status ekf_get_state(ekf_handle h, double* out /* N */);
ekf_status ekf_set_state(ekf_handle h, const double* in /* N */);
ekf_status ekf_get_cov(ekf_handle h, double* out /* N*N row-major */);
ekf_status ekf_set_cov(ekf_handle h, const double* in /* N*N row-major */);
ekf_status ekf_get_init_flag(ekf_handle h, int* flag);  /* landmark_init_flag, ekf_slam.hpp:65 */
ekf_status ekf_set_init_flag(ekf_handle h, int flag);
/* ---- execution forms (test / measurement hook; a caller never needs it) -----------------------------------------
 * Every entry point computes ONE function -- the reference's -- but the library holds several launch structures
 * ("forms") for it and picks among them by map size and pool size (DESIGN.md section 4, table "path selection").
 * All exact forms are bit-identical to each other; the tests switch them off one by one and compare bit for bit.
 * A bit set = the form may be taken where it applies (default: EKF_FORMS_DEFAULT = all but the ALWAYS hook). */
typedef enum {
    /* N = 3 + 2n <= 104 (the reference's own n = 20): a whole measurement() / data_association() call, a whole step of
     * a pool (while 3 + 2*(known_count + readings) <= 104) or a whole run of a known-association log is ONE launch with
     * Sigma resident in LDS (ekf_small.hip).  Off: the multi-kernel chain. */
    EKF_FORM_SMALL_MAP = 1u << 0,
    /* (1u << 1: retired in round 4.  It was EKF_FORM_FUSED_CORRECTION -- gain + state + covariance of a correction in one
     * launch that wrote Sigma - K(H Sigma) out of place into a second N x N buffer; tools/forms_ab.py measured it 2.5-4.7x
     * behind the call-fused forms on measurement() and 1.3-1.5x behind them on data_association() at every map size, so
     * the kernels and the second buffer were deleted.  The bit is ignored.) */
    /* beyond the small-map path: measurement() as TWO launches per call whatever the number of visible landmarks --
     * the gains K_v and rows H_v Sigma of all the call's corrections from two thin panels of Sigma, then ONE
     * read-modify-write pass in which every element takes its V rank-2 corrections in order: 16 N^2 bytes per CALL
     * (per 8 corrections) instead of per landmark (ekf_callfused.hip); a single filter's data_association() as one launch
     * per reading + one pass per call (ekf_assocfused.hip).  Off: one covariance stream per landmark -- the eager
     * contract stream bench.py quotes `value` / `roofline` on. */
    EKF_FORM_CALL_FUSED = 1u << 2,
    /* data_association() appends landmarks in discovery order, so its corrections are exactly confined to the leading
     * 3 + 2*known_count block of the state: stream only that block.  Off: full width. */
    EKF_FORM_ACTIVE_PREFIX = 1u << 3,
    /* pools, ekf_batch_run_unknown beyond the LDS-resident path, <= 8 reading slots per step: one launch per STEP (a
     * workgroup per filter scores, decides and builds the gains against the stored covariance minus the step's pending
     * pairs; ekf_stepfused.hip).  Off: four launches per reading slot. */
    EKF_FORM_STEP_FUSED = 1u << 4,
    /* ... and when the discovered prefixes are big, the step's covariance pass as a second launch spread over the chip. */
    EKF_FORM_STEP_SPLIT_PASS = 1u << 5,
    /* delayed mode, ekf_batch_run_known: the two corrections of a step in ONE gain launch (pending factors read once). */
    EKF_FORM_DELAYED_PAIR = 1u << 6,
    /* narrow maps: P consecutive rows streamed as one virtual row that fills the 256-lane strips (k_rank2_packed). */
    EKF_FORM_ROW_PACKING = 1u << 7,
    /* delayed mode: the strip-form flush (V strip in LDS) beyond 40 pending vectors on pools that fill the chip. */
    EKF_FORM_STRIP_FLUSH = 1u << 8,
    /* test hook: the strip-form flush on pools of any size, for any count <= 80 vectors. */
    EKF_FORM_STRIP_FLUSH_ALWAYS = 1u << 9,
    /* delayed mode, ekf_batch_run_known: the flush also writes the COLUMNS of Sigma that the next corrections' K = Sigma H^T
     * S^-1 (ekf_slam.cpp:178) will read -- columns 0..2 and the two columns of every landmark in the next corrections of
     * the device-resident log -- as contiguous rows of a column panel, the gain kernels read them coalesced instead of as
     * 16-KB-strided sectors, and prediction() keeps columns 0..2 current in the panel (coalesced) instead of in the matrix.
     * Same values from another address: bit-identical.  Off: columns are gathered from the matrix. */
    EKF_FORM_COLUMN_PANEL = 1u << 10,
    /* test hook: the panel plans ONE landmark per flush period, so panel rows and matrix gathers are mixed in one launch. */
    EKF_FORM_COLUMN_PANEL_ONE_SLOT = 1u << 11,
    /* pools' delayed data_association() (ekf_batch_run_unknown in delayed mode): a launch in front of every step guesses each
     * reading's winner (the landmark nearest to where the reading lands) and rebuilds "stored covariance minus the pairs of
     * earlier steps" for the guessed landmarks' rows / columns ONCE per step; the step kernel continues from it where its own
     * decision agrees and rebuilds from scratch where it does not -- the pending store is read once per step instead of once
     * per reading.  Same operations in the same order: bit-identical.  Off: every reading rebuilds. */
    EKF_FORM_STEP_SPECULATE = 1u << 12,
    /* with the column panel (delayed known-association runs, paired gain launches): the rows and columns of Sigma at the pose
     * indices and at every planned landmark are KEPT as they stand after each launch that rebuilt them, and the next launch
     * that meets them folds only the pending vectors appended since -- a robot corrects the same few landmarks step after
     * step, so a gain launch reads 4 factor vectors instead of all pending ones.  prediction() maps the kept vectors like
     * the rest of Sigma.  The same quantities in another association of the sums: equal to the run without it to rounding
     * (1e-10 in the tests, where the delayed mode itself sits 1e-10 from the eager run), not bit for bit.  Off: every launch rebuilds from the stored entries. */
    EKF_FORM_CURRENT_COLUMNS = 1u << 13,
    /* pools with many more rank-2 tiles than CUs stream the eager correction as RESIDENT workgroups that take their tiles from
     * one queue (an atomicAdd per tile) instead of a grid of short-lived ones: the dispatcher deals a fixed eighth of a grid to
     * each XCD, and XCDs / CUs do not stream at the same rate (tools/micro/strip_walk.hip).  Speed only: same arithmetic. */
    EKF_FORM_TILE_QUEUE = 1u << 14,
    /* eager pools whose single correction takes the tile queue apply ALL corrections of a step (two or more active slots) in
     * ONE launch, tile batch by tile batch: a resident workgroup sweeps its batch once per correction and re-loads what it
     * stored itself while the lines are still in its XCD's L2 (ekf::k_rank2_chain; the factors of the step come from the
     * call-fused factor kernel).  Each correction still reads and writes every element through the memory system; same
     * arithmetic in the same order: bit-identical.  Off: one launch per correction. */
    EKF_FORM_STEP_CHAIN = 1u << 15,
    EKF_FORMS_DEFAULT = ((1u << 9) - 1) | (1u << 10) | (1u << 12) | (1u << 13) | (1u << 14) | (1u << 15)
} ekf_form;
ekf_status ekf_set_forms(ekf_handle h, unsigned forms);
ekf_status ekf_get_forms(ekf_handle h, unsigned* forms);
ekf_status ekf_batch_set_forms(ekf_batch_handle hb, unsigned forms);
ekf_status ekf_batch_get_forms(ekf_batch_handle hb, unsigned* forms);
/* Test hook: covariance passes of each form this pool has launched since it was created --
 * counts[0] plain flush, [1] strip-form flush, [2] paired delayed gain launches, [3] call-fused passes,
 * [4] per-landmark rank-2 streams, [5] step-fused launches with a separate pass, [6] mirrored flushes (symmetric
 * option of ekf_set_update_mode), [7] delayed gain launches that read the column panel (EKF_FORM_COLUMN_PANEL). */
ekf_status ekf_batch_form_counts(ekf_batch_handle hb, long long counts[8]);
/* Test hook of EKF_FORM_STEP_SPECULATE, since creation / ekf_batch_reset: out[0] readings of delayed unknown-association
 * steps whose decision (an active re-observation) was compared with the guesses of the launch in front, out[1] those that
 * found their winner among the guesses and continued from its rebuilt rows (out[1] <= out[0]; both 0 with the form off). */
ekf_status ekf_batch_spec_counts(ekf_batch_handle hb, long long out[2]);
/* Experiment / test hook of EKF_FORM_STEP_CHAIN.  tiles_per_batch: 16-row x 512-column tiles per queue item (0 = automatic:
 * 1).  policy: 0 = automatic; 16 + bits = non-temporal accesses where a bit is set, plain otherwise: 1 the first sweep's
 * loads, 2 the stores of every sweep but the last, 4 the re-loads, 8 the last sweep's stores.  Speed only. */
ekf_status ekf_batch_set_chain(ekf_batch_handle hb, int tiles_per_batch, int policy);
/* since the pool was created: out[0] chained launches, out[1] correction passes they applied (both 0 with the form off) */
ekf_status ekf_batch_chain_counts(ekf_batch_handle hb, long long out[2]);

/* Active-set covariance update (opt-in, default 0; reported separately from the dense contract path):
 * the eager correction streams only the rows of the TOUCHED set -- the pose rows and the rows of landmarks
 * that have ever been corrected.  Every other row has K(r,:) = 0 exactly (its landmark still carries the
 * constructor covariance and is decoupled from everything), so the result is bit-identical for finite
 * states while the traffic drops from 2*8*N^2 to 2*8*N*(3 + 2*touched) bytes per correction. */
ekf_status ekf_set_active_set(ekf_handle h, int enable);
ekf_status ekf_batch_set_active_set(ekf_batch_handle hb, int enable);
/* Size of every filter's touched set (landmarks corrected at least once): counts_out[B]. */
ekf_status ekf_batch_get_touched(ekf_batch_handle hb, int* counts_out);
/* Diagnostics of the two-launch measurement() call: while enabled, lane 0 of the control wave (row 0) and of the first
 * slice wave (row 1) of workgroup 0 of k_call_factors stamp the 100 MHz wall clock at their phase boundaries.  out (nullable)
 * receives the stamps of the LAST call, [2][64] (slots: 0 start, 1 gathers issued, 2 prediction folded, then per
 * correction t at 3 + 5t: barrier passed, terms / panel update done, second barrier passed, gains done; 60 loop done). */
ekf_status ekf_phase_trace(ekf_handle h, int enable, long long* out);
/* Test hook of the device error word: a one-thread kernel raises it the way a kernel that gave up would (a bounded
 * in-kernel hand-off that never arrived).  The call itself returns EKF_OK; every LATER entry point of the handle must
 * fail with EKF_ERR_HIP (the word is sticky: results behind it are not to be used). */
ekf_status ekf_test_raise_device_error(ekf_handle h);
/* Blocks until every kernel queued on the handle's stream has finished. */
ekf_status ekf_sync(ekf_handle h);
/* Device bytes the filter holds: the exact sum of its live device allocations (as ekf_batch_device_bytes). */
ekf_status ekf_device_bytes(ekf_handle h, size_t* bytes);
/* Measurement hook (off by default): brackets every covariance-streaming launch (class 0: fused correction, rank-2
 * stream, decision + correction) and every Mahalanobis scoring launch (class 1) of this filter with HIP events on
 * its stream.  ekf_get_profile synchronises and returns the summed kernel milliseconds and launch counts per class
 * since profiling was switched on. */
ekf_status ekf_set_profiling(ekf_handle h, int enable);
ekf_status ekf_get_profile(ekf_handle h, double ms[2], long long launches[2]);

/* ---- batch of independent filters (BASELINE.json configs[4]) -------
 * Each filter is exactly one EKF_SLAM object; they share nothing.  Inputs are a compact
 * known-association log (visible readings only, ascending landmark index -- the order of the
 * loop at ekf_slam.cpp:132), uploaded once so the timed region starts with inputs in HBM. */

typedef struct {
    int T;               /* steps; step t = prediction(twist[t]) + measurement(readings[t])   */
    int vmax;            /* reading slots per step                                             */
    const double* twist; /* [T][B][2]  (dtheta, dx)                                            */
    const int* lm_idx;   /* [T][B][vmax] landmark index per slot, ascending, -1 ends the list  */
    const double* z_xy;  /* [T][B][vmax][2] robot-frame (x, y) readings                        */
    const double* init_xy; /* [B][2n] sensor_reading of the FIRST measurement() call (:113-128) */
} ekf_known_log;

typedef struct {
    double elapsed_ms;        /* HIP-event time of the whole run on the batch's stream         */
    double rank2_ms;          /* sum of the durations of the covariance passes (time_kernels): */
                              /* eager: the rank-2 kernel; delayed mode: the flush kernel      */
    long long rank2_launches; /* covariance passes in the run (eager: one per correction slot) */
    long long corrections;    /* landmark corrections applied over all filters                 */
    long long filter_steps;   /* (prediction + measurement) pairs over all filters             */
    double rank2_bytes_per_launch; /* algorithmic bytes of one pass: (filters touched) * 2*8*N^2 */
} ekf_run_stats;

ekf_status ekf_batch_create(int B, int n, const ekf_params* params, int device, ekf_batch_handle* out);
ekf_status ekf_batch_destroy(ekf_batch_handle hb);
/* Re-initialise every filter to the constructor state (ekf_slam.cpp:27-53). */
ekf_status ekf_batch_reset(ekf_batch_handle hb);
/* Device bytes the batch holds (covariance pool + state + scratch + uploaded log): the exact sum of its live device
 * allocations, the delayed mode's factor store and column panel included. */
ekf_status ekf_batch_device_bytes(ekf_batch_handle hb, size_t* bytes);
ekf_status ekf_batch_upload_known_log(ekf_batch_handle hb, const ekf_known_log* log);
/* Runs steps [t_begin, t_end) of the uploaded log for all filters on the batch's stream and
 * waits for completion.  time_kernels != 0 brackets every rank-2 launch with HIP events. */
ekf_status ekf_batch_run_known(ekf_batch_handle hb, int t_begin, int t_end, int time_kernels,
                               ekf_run_stats* stats);

/* Unknown-association log: per step one twist and up to jmax robot-frame circle centres per filter --
 * the node loop of nuslam/src/unknown_data_assoc.cpp:300-323 (prediction(twist), then
 * data_association(measures, known_list)) for B independent robots. */
typedef struct ekf_unknown_log {
    int T;                 /* steps */
    int jmax;              /* measurement slots per (step, filter) */
    const double* twist;   /* [T][B][2]  (angular, linearX) */
    const int* count;      /* [T][B]     measurements of filter b in step t, 0..jmax */
    const double* meas_xy; /* [T][B][jmax][2] robot-frame (x, y); slots >= count are ignored */
} ekf_unknown_log;
ekf_status ekf_batch_upload_unknown_log(ekf_batch_handle hb, const ekf_unknown_log* log);
/* Runs steps [t_begin, t_end) of the uploaded unknown-association log: per step prediction()
 * (ekf_slam.cpp:55-106), then per measurement slot the Mahalanobis scores (:217-276), the
 * gate decision / landmark initialisation (:293-330) and the correction (:331-390) of every filter
 * that has a measurement in the slot.  Each filter's known_count (the leading run of its
 * known_list, :281-288) lives on the device and carries over between runs until ekf_batch_reset.
 * In delayed mode (ekf_batch_set_update_mode(k > 0)) with at most 8 reading slots per step, the pairs of a step stay
 * pending across steps -- every reading is scored and corrected against the stored covariance minus ALL pending pairs,
 * Sigma is rewritten once per floor(k / jmax) steps -- with the mode's tolerance (1e-9; decisions identical in every
 * test); otherwise pending delayed corrections are flushed first and the run is eager.  stats->corrections counts the
 * corrections actually applied (decided on the device). */
ekf_status ekf_batch_run_unknown(ekf_batch_handle hb, int t_begin, int t_end, int time_kernels,
                                 ekf_run_stats* stats);
/* The batch twin of the caller-owned known_list argument of data_association(): sets every filter's known_count
 * (the leading run of its known_list, ekf_slam.cpp:281-288) to counts[b] in 0..n -- e.g. to continue with unknown
 * association on a map built through the known-association path, whose first call initialises all n landmarks
 * (:113-128).  Landmarks below the count are treated as possibly corrected (no discovered-prefix shortcut). */
ekf_status ekf_batch_set_known_counts(ekf_batch_handle hb, const int* counts);
/* known_count of every filter: out[B]. */
ekf_status ekf_batch_get_known_counts(ekf_batch_handle hb, int* out);
/* Decisions of the uploaded unknown log's steps run so far: out = [T][B][jmax], landmark index
 * corrected, -1 = measurement dropped (:330), -2 = no measurement in the slot / step not run. */
ekf_status ekf_batch_get_decisions(ekf_batch_handle hb, int* out);

ekf_status ekf_batch_get_state(ekf_batch_handle hb, int b, double* out /* N */);
ekf_status ekf_batch_get_cov(ekf_batch_handle hb, int b, double* out /* N*N row-major */);
/* All poses at once: out = [B][3] (theta, x, y) -- the Monte-Carlo read-back. */
ekf_status ekf_batch_get_poses(ekf_batch_handle hb, double* out);
/* order-independent digest of every filter's state and covariance (device-side reduction):
 * out[0] = sum state, out[1] = sum |state|, out[2] = sum sigma, out[3] = sum |sigma| */
ekf_status ekf_batch_checksum(ekf_batch_handle hb, double out[4]);

/* Tuning knobs of the covariance rank-2 kernel: rows per workgroup, non-temporal access (0/1),
 * rows per load/store group (2, 4, 8 or 16).  0 (nontemporal: < 0) restores the automatic choice.
 * Results do not depend on them, bit for bit. */
ekf_status ekf_batch_set_tuning(ekf_batch_handle hb, int rows_per_block, int nontemporal, int group_rows);
/* Report hooks of the launch a full-width eager correction of this pool makes (bench.py ties its PMC traffic record to the
 * kernel's name); all three read the one plan the launcher launches from.
 * _packing: P, the rows the row-packed kernel streams as one virtual row; 1 = the plain kernel (EKF_FORM_ROW_PACKING).
 * _variant: P == 1: the instantiation ekf::k_rank2<group_rows, nontemporal, threads> and its rows per workgroup;
 *           P > 1: ekf::k_rank2_packed<group_rows, nontemporal>, threads = 256, and its VIRTUAL rows per workgroup.
 * _resident: the launch runs as resident workgroups on one tile queue (ekf::k_rank2_queue<...>, EKF_FORM_TILE_QUEUE);
 *           0 whenever P > 1 (the packed kernel is taken first). */
ekf_status ekf_batch_rank2_variant(ekf_batch_handle hb, int* group_rows, int* nontemporal, int* threads,
                                   int* rows_per_block);
ekf_status ekf_batch_rank2_resident(ekf_batch_handle hb, int* resident);
ekf_status ekf_batch_rank2_packing(ekf_batch_handle hb, int* P);
ekf_status ekf_set_tuning(ekf_handle h, int rows_per_block, int nontemporal, int group_rows);

/* ---- on-device Monte-Carlo inputs and consistency statistics --------
 * Generates the known-association log of every filter ON THE DEVICE from the noise model of the
 * reference's simulator (nurtlesim/src/tube_world.cpp:191-227,369-414; constants
 * nurtlesim/config/noise_param.yaml:2-11) and the caller's odometry marshalling
 * (nuslam/src/slam.cpp:173-176), instead of uploading it.  Every random number is a pure function of
 * (seed, first_filter_id + b, step, kind, k), so shards of one job are reproducible independently. */
typedef struct {
    unsigned long long seed;
    long long first_filter_id;   /* global id of filter 0 of this batch (multi-GPU sharding)          */
    double v_cmd, w_cmd;         /* commanded twist (m/s, rad/s)                                       */
    double vx_std, the_std;      /* noise_param.yaml:3,5   noise on the commanded twist                */
    double slip_min, slip_max;   /* noise_param.yaml:6-7   wheel slip ~ U(slip_min, slip_max)          */
    double sensor_std;           /* noise_param.yaml:8-9   per-axis reading noise                      */
    double max_visible_dis;      /* noise_param.yaml:10    visibility radius                           */
    double wheel_base, wheel_radius; /* rigid2d/config/fake_turtle_param.yaml:6-7                     */
    int ticks_per_step;          /* 100 Hz simulator ticks per 10 Hz filter step (10)                  */
} ekf_sim_params;
void ekf_default_sim_params(ekf_sim_params* out);
/* world_xy: [n][2] landmark positions (host).  Replaces any uploaded log; T steps, vmax reading slots. */
ekf_status ekf_batch_simulate_known_log(ekf_batch_handle hb, const ekf_sim_params* sp, const double* world_xy,
                                        int T, int vmax);
/* Copies the device-resident log back (any pointer may be NULL): shapes as in ekf_known_log, plus
 * true_pose [T][B][3] = simulated ground truth (theta, x, y) AFTER step t (simulated logs only). */
ekf_status ekf_batch_download_log(ekf_batch_handle hb, double* twist, int* lm_idx, double* z_xy, double* init_xy,
                                  double* true_pose);

/* 2-D lidar of the simulator (publishScan, nurtlesim/src/tube_world.cpp:451-577). */
typedef struct ekf_lidar_params {
    int n_beams;          /* 360, tube_world.cpp:452                                      */
    double range_std;     /* nurtlesim/config/noise_param.yaml: range_std 0.005           */
    double range_max;     /* 3.5, tube_world.cpp:476                                      */
    double border_width;  /* tube_param.yaml: world_border_width 2.0 (square wall)        */
    double tube_radius;   /* tube_param.yaml: tube_radius 0.0762                          */
    /* 0 (default): clean ray geometry -- nearest of the wall hit, range_max and the first intersection of the beam with
     * every tube.  1: publishScan's own procedure, step for step (tube_world.cpp:496-570): a tube is looked at only by the
     * beams inside a bearing window of 2 atan2(radius, range_min) around it (:503,533-562), and the hit is the nearer of
     * the two intersections of the LINE through the robot and the beam's end point with the tube's circle
     * (getLineCircleIntersection, :420-450).  The two agree to rounding wherever no tube is closer than
     * radius / sin(atan2(radius, range_min)) = 0.142 m to the lidar (tests/test_host.py); closer tubes the window clips. */
    int model;
    double range_min;     /* 0.12, tube_world.cpp:475 (model 1: the bearing window)      */
} ekf_lidar_params;
void ekf_default_lidar_params(ekf_lidar_params* out);
/* Unknown-association inputs generated ON THE DEVICE for every filter of the batch (replaces any
 * uploaded unknown log): the simulated trajectory / odometry twists of ekf_batch_simulate_known_log, and
 * per (step, filter) up to jmax (<= 64) robot-frame measurements from
 *   lidar == NULL : the fake sensor -- noisy positions of the landmarks within max_visible_dis, shuffled
 *                   (the scan_measures vector of nuslam/src/unknown_data_assoc.cpp:309-320);
 *   lidar != NULL : a simulated laser scan per (step, filter) pushed through the batched circle
 *                   fitting (nuslam/src/landmarks.cpp:141 -> rigid2d::CircleFitting), scans never
 *                   leaving the device. */
ekf_status ekf_batch_simulate_unknown_log(ekf_batch_handle hb, const ekf_sim_params* sp,
                                          const ekf_lidar_params* lidar, const double* world_xy, int T, int jmax);
/* Copies the device-resident unknown log back (any pointer may be NULL): shapes as in ekf_unknown_log,
 * true_pose [T][B][3] for simulated logs. */
ekf_status ekf_batch_download_unknown_log(ekf_batch_handle hb, double* twist, int* count, double* meas_xy,
                                          double* true_pose);
/* Stand-alone scan simulator: scan s is taken from poses[s] = (theta, x, y) with the noise stream of
 * filter sp->first_filter_id + s at step `step`; ranges_out = [S][n_beams]. */
ekf_status ekf_simulate_scans(int device, const ekf_sim_params* sp, const ekf_lidar_params* lidar,
                              const double* world_xy, int n, const double* poses, int S, int step,
                              double* ranges_out);

/* Consistency of the batch against the simulated truth of step t:
 * out = {mean NEES (3 dof), max NEES, RMSE position, RMSE heading, mean trace of the pose covariance,
 *        fraction of filters with NEES < 7.815 (95 % chi-square bound, 3 dof)}. */
ekf_status ekf_batch_mc_stats(ekf_batch_handle hb, int t, double out[6]);

/* Covariance update mode.  0 (default) = EAGER: every landmark correction streams Sigma once
 * (16 N^2 bytes) -- the contract path the roofline is quoted on.  k > 0 = DELAYED rank-2k update
 * (SURVEY.md section 8(f) f2): up to k corrections are kept as low-rank factors
 * (Sigma = Sigma_base - sum K_j (H Sigma)_j), the rows/columns a correction needs are rebuilt on the
 * fly, prediction() maps the factors, and Sigma is rewritten once per k corrections (and before any
 * call that reads it: get_cov, checksum, clone, maha_scores; batch pools also before unknown-association runs).
 * A single filter's data_association() stays delayed too: the Mahalanobis scores are taken against Sigma_base minus
 * the pending pairs, the winner's correction is appended like any other.  Same results to rounding (tested at 1e-9);
 * k is capped at 64.
 * symmetric_gather != 0 (delayed mode only; opt-in, reported separately): the SYMMETRIC option.  The reference never
 * symmetrises Sigma, but (I - KH)Sigma keeps it symmetric to rounding (measured asymmetry 1e-18 relative, SURVEY.md
 * App. A2), and this option uses that:
 *   - the gain step takes Sigma H^T as (H Sigma)^T: only the rows Sigma(c, .) are rebuilt, from coalesced base rows and
 *     the V half of the pending store (no 16-KB-strided column gathers, half of the factor read);
 *   - for N >= 256 the flush forms the tiles on and above the diagonal only and writes each tile above it twice, in place
 *     and mirrored (4 N^2 bytes read + 8 N^2 written instead of 8 + 8; half of the multiply-adds): Sigma_base is then
 *     symmetric to the bit outside the 32 x 32 diagonal squares;
 *   - inside a known-association pool run the tiles on and above the diagonal ARE the covariance between flushes
 *     (prediction() keeps up the rows 1, 2 and leaves their strided column images to the next mirroring flush; every run
 *     returns with the full matrix restored).
 * Not the reference's operands -- do not use it on a covariance that was set deliberately asymmetric -- but within the
 * mode's 1e-9 (tests/test_gpu_delayed.py: 3.7e-13 on the bench configuration). */
ekf_status ekf_set_update_mode(ekf_handle h, int max_pending_corrections, int symmetric_gather);
ekf_status ekf_batch_set_update_mode(ekf_batch_handle hb, int max_pending_corrections, int symmetric_gather);
/* ---- dense general-F covariance propagation, fp32 on the matrix cores (BASELINE.json configs[3]) ----
 * Sigma <- F * Sigma * F^T + Q for an ARBITRARY dense F: the reference's expression
 * `sigma = At*sigma*At.t() + Q` (ekf_slam.cpp:101-102) as Armadillo executes it (two dense N^3
 * products).  The filter's own At = I + A never needs this (ekf_predict is O(N)); the entry point
 * serves motion models with a dense Jacobian and is checked against fp64 (tolerance 1e-4 per block).
 * All matrices are row-major N x N fp32 host buffers. */
typedef struct ekf_dense_s* ekf_dense_handle;
ekf_status ekf_dense_create(int N, int device, ekf_dense_handle* out);
ekf_status ekf_dense_destroy(ekf_dense_handle h);
/* Any of F, Sigma, Q may be NULL to keep the current device contents (initially all zero). */
ekf_status ekf_dense_set(ekf_dense_handle h, const float* F, const float* Sigma, const float* Q);
/* Applies the propagation `iterations` times; elapsed_ms (nullable) = HIP-event time of the launches. */
ekf_status ekf_dense_propagate(ekf_dense_handle h, int iterations, double* elapsed_ms);
ekf_status ekf_dense_get_sigma(ekf_dense_handle h, float* out);
/* Test / report hook: how one product of this handle is launched -- ld (N rounded up to 128), tiles = ld / 128 per
 * side, n_big = 256 x 128 tiles run by the main kernel (whole rounds of resident workgroups), n_tail = 128 x 128 tiles
 * cut into 64 x 64 quarters for the tail kernel behind it (what is left of the big-tile list, and the bottom strip of an
 * ld that is an odd multiple of 128).  Any pointer may be NULL. */
ekf_status ekf_dense_launch_info(ekf_dense_handle h, int* ld, int* tiles, int* n_big, int* n_tail);
/* ... and which kernel computes which 128 x 128 block of the result: map[tiles * tiles], row-major over blocks,
 * 0 = main kernel, 1 = tail kernel (the tests sample rows inside tail tiles with it). */
ekf_status ekf_dense_tile_map(ekf_dense_handle h, unsigned char* map);

/* ---- dense general-F covariance propagation, fp64 on the matrix cores ----
 * The same Sigma <- F * Sigma * F^T + Q with every value and every accumulation in fp64 (v_mfma_f64_16x16x4_f64), so a
 * caller with an fp64 covariance keeps the library's contract: tests/test_gpu_dense64.py holds it to 1e-12 relative per
 * block against numpy fp64 (1e-9 = FP64_TOL against the checker's prediction()), integer operands bit-exact.
 * A separate handle type, so fp32 and fp64 buffers cannot be mixed.  Same meaning and status codes as the fp32 functions
 * (N <= 0 or a NULL out: EKF_ERR_INVALID; no device, or a device that is not gfx950: EKF_ERR_NO_DEVICE; no CPU path).
 * Device matrices are ld x ld with ld = N rounded up to 128 and zero padding; the handle holds four of them
 * (F, Sigma, the product F * Sigma, Q): 32 ld^2 bytes, about 3.3 GB at N = 10003 (ld = 10112) -- plus, for the measurement
 * update below, the state vector and one correction's operands: 8 ld (1 + 2 * 64) + 33 KB, i.e. 10.5 MB at N = 10003.
 * The update's panels and partial sums live in the product buffer, which is dead between propagations; only a small
 * handle (ld below about 3000), where they do not fit, allocates them separately (46 MB at N = 2003, less below).
 * All host matrices are row-major N x N fp64. */
typedef struct ekf_dense64_s* ekf_dense64_handle;
ekf_status ekf_dense64_create(int N, int device, ekf_dense64_handle* out);
ekf_status ekf_dense64_destroy(ekf_dense64_handle h);
/* Any of F, Sigma, Q may be NULL to keep the current device contents (initially all zero). */
ekf_status ekf_dense64_set(ekf_dense64_handle h, const double* F, const double* Sigma, const double* Q);
/* Applies the propagation `iterations` times; elapsed_ms (nullable) = HIP-event time of the launches. */
ekf_status ekf_dense64_propagate(ekf_dense64_handle h, int iterations, double* elapsed_ms);
ekf_status ekf_dense64_get_sigma(ekf_dense64_handle h, double* out);
/* Test / report hook: ld, tiles = ld / 128 per side, n_big = 128 x 128 tiles run by the main kernel (whole rounds of two
 * resident workgroups per CU), n_tail = 128 x 128 tiles left over, cut into 64 x 64 quarters for the tail kernel behind
 * it.  Any pointer may be NULL. */
ekf_status ekf_dense64_launch_info(ekf_dense64_handle h, int* ld, int* tiles, int* n_big, int* n_tail);
/* ... and which kernel computes which 128 x 128 block: map[tiles * tiles], 0 = main kernel, 1 = tail kernel. */
ekf_status ekf_dense64_tile_map(ekf_dense64_handle h, unsigned char* map);
#define EKF_DENSE64_MAX_M 64
/* state vector of the handle (N doubles, initially zero) */
ekf_status ekf_dense64_set_state(ekf_dense64_handle h, const double* x /* N */);
ekf_status ekf_dense64_get_state(ekf_dense64_handle h, double* out /* N */);
/* One measurement update with an arbitrary dense Jacobian -- ekf_slam.cpp:178,186,191-192 for general operands:
 *   T = H Sigma (m x N, rows of Sigma)      U = Sigma H^T (N x m, COLUMNS of Sigma: Sigma is never symmetrised)
 *   S = T H^T + R      K = U S^-1      state += K nu      Sigma <- Sigma - K T   ( = (I - K H) Sigma to rounding )
 *   *nis_out = nu^T S^-1 nu   (the score of calculate_maha_dis, :267-269)
 * H: m x N row-major, R: m x m row-major (need not be diagonal or symmetric), nu: m (NULL: state untouched, nis_out
 * must then be NULL), 1 <= m <= min(N, EKF_DENSE64_MAX_M).  Synchronous.  elapsed_ms (nullable) = HIP-event time of
 * the launches only (no H2D of H / R / nu).
 * S is inverted by elimination with partial pivoting in fp64.  A zero or non-finite pivot (or a non-finite entry of S
 * or of S^-1) returns EKF_ERR_STATE and leaves state and Sigma exactly as they were: the verdict is a device word the
 * writing launches read before their first store.  The padding of Sigma stays zero, so ekf_dense64_propagate and
 * ekf_dense64_correct alternate without Sigma leaving the device.  Bad arguments (NULL handle, NULL H or R, m < 1,
 * m > EKF_DENSE64_MAX_M, m > N, nis_out without nu) return EKF_ERR_INVALID before the device is looked at.
 * No floating-point atomics: the same inputs give the same bits every time.  The wrapping of an angle in nu or in the
 * state (:183,187) is the caller's business: the entry point is model-free. */
ekf_status ekf_dense64_correct(ekf_dense64_handle h, int m, const double* H, const double* R, const double* nu,
                               double* nis_out, double* elapsed_ms);

/* Scoring of J candidate measurements against the covariance WITHOUT changing it -- the reference's calculate_maha_dis
 * (ekf_slam.cpp:217-276: psi = Hj*sigma*Hj.t() + R, d = nu^T psi^-1 nu), called once per known landmark by
 * data_association() (:300-314) before it decides which one to correct -- for J arbitrary dense m x N Jacobians at once:
 *   S_j = (H_j Sigma) H_j^T + R_j      nis_j = nu_j^T S_j^-1 nu_j
 * with the operand order of ekf_dense64_correct (rows of Sigma weighted by H_j first; Sigma is never symmetrised) and
 * the same elimination with partial pivoting (one device routine serves both).
 * H: [J][m][N] row-major; R: [J][m][m], or one [m][m] for all candidates when r_shared != 0; nu: [J][m], NULL allowed
 * only when nis_out is NULL; nis_out [J], S_out [J][m][m] and flag_out [J] are each nullable, but not all three.
 * 1 <= m <= min(N, EKF_DENSE64_MAX_M), J >= 1, J * m <= EKF_DENSE64_SCORE_MAX_ROWS.  A NULL handle / H / R, a bad J or m,
 * nis_out without nu or no output at all return EKF_ERR_INVALID before the device is looked at.
 * Read-only: Sigma, the state and every operand of propagate / correct are bit for bit what they were (the product
 * buffer F * Sigma, dead between propagations, serves as workspace, as it does for correct).
 * UNLIKE ekf_dense64_correct, where there is one S and nothing to go on with, a singular or non-finite S_j is not an
 * error of the call: that candidate gets flag 1 and nis = NaN (S_out holds what was summed), the call returns EKF_OK and
 * every other candidate's outputs are unaffected.
 * A candidate's outputs do not depend on what else is in the call: alone or at any position of any batch with the same
 * m, with R shared or replicated, they are the same bits; and the same from run to run (no floating-point atomics).
 * The argmin and the gates are the caller's: INTEGRATION.md shows the reference's rule (:293-330) next to this call.
 * Buffers for the candidates are allocated by the first call of a handle and grow with larger calls (the stacked
 * Jacobians, 512 ld bytes per group of floor(64 / m) candidates; 2.1 MB of operands and results; partial blocks that do
 * not fit the product buffer); a failure there returns EKF_ERR_NOMEM and leaves the handle as it was.
 * Synchronous, on the handle's stream.  elapsed_ms (nullable) = HIP-event time of the three launches only. */
#define EKF_DENSE64_SCORE_MAX_ROWS 2048     /* J * m of one call */
ekf_status ekf_dense64_score(ekf_dense64_handle h, int J, int m,
                             const double* H,     /* [J][m][N], row-major, dense */
                             const double* R,     /* [J][m][m], or [m][m] when r_shared != 0 */
                             int r_shared,
                             const double* nu,    /* [J][m] innovations; NULL allowed only when nis_out is NULL */
                             double* nis_out,     /* [J]  nu_j^T S_j^-1 nu_j          (nullable) */
                             double* S_out,       /* [J][m][m]  S_j = H_j Sigma H_j^T + R_j   (nullable) */
                             int* flag_out,       /* [J]  0 = scored, 1 = S_j singular or not finite (nullable) */
                             double* elapsed_ms); /* HIP-event time of the launches only (nullable) */

/* Block-structured prediction: the motion model every SLAM caller has -- a dynamic block of r states anywhere in the
 * vector with an arbitrary r x r Jacobian, everything else static.  The reference's prediction() (ekf_slam.cpp:76-102)
 * builds At = eye + A with A non-zero in the pose rows only and Q non-zero in the pose block only; this call is that
 * shape for a general model.  It gives what ekf_dense64_propagate(h, 1, ..) gives for `sigma = At*sigma*At.t() + Q`
 * (:101-102) in its association (At*sigma)*At.t() + Q with
 *   F = identity with Fr written into [first, first + r)^2        Q = zero with Qr written into the same square
 * that is, with b = [first, first + r):
 *   Sigma[b, j] <- Fr Sigma[b, j]   for every column j outside b   (rows of Sigma)
 *   Sigma[i, b] <- Sigma[i, b] Fr^T for every row i outside b      (COLUMNS of Sigma: Sigma is never symmetrised)
 *   Sigma[b, b] <- (Fr Sigma[b, b]) Fr^T + Qr                      (the inner product rounded to fp64 first)
 *   state[first + k] += dx[k]       when dx is given               (state = state + update, :99)
 * and no entry outside the block's rows and columns is written: 32 r N bytes move instead of the two N^3 products.
 * Fr: r x r row-major; Qr: r x r row-major, NULL = zero; dx: r, NULL = state untouched.
 * 1 <= r <= min(N, EKF_DENSE64_MAX_R), 0 <= first, first + r <= N.  A NULL handle or Fr, or a bad first or r, returns
 * EKF_ERR_INVALID before the device is looked at.
 * The F and Q stored by ekf_dense64_set are neither read nor changed, the padding of Sigma and of the state stays zero,
 * so the two ways of predicting alternate freely with ekf_dense64_correct and ekf_dense64_score without Sigma leaving
 * the device.  Memory: 66 KB of operands (Fr, Qr, dx) allocated with the handle; nothing of size ld^2, no workspace.
 * One launch, no floating-point atomics.  Every dot product has exactly r terms, accumulated from +0 in ascending k
 * with one fused multiply-add per term, an order that does not depend on N, ld, first or the launch geometry: the same
 * block data gives the same bits wherever the block sits, whatever N is, on every run.
 * The non-linear motion function that produces dx and any wrapping of an angle in the state stay with the caller: the
 * entry point is model-free.  Synchronous, on the handle's stream.  elapsed_ms (nullable) = HIP-event time of the
 * launch only (no H2D of Fr / Qr / dx). */
#define EKF_DENSE64_MAX_R 64
ekf_status ekf_dense64_propagate_block(ekf_dense64_handle h, int first, int r,
                                       const double* Fr,    /* r x r row-major */
                                       const double* Qr,    /* r x r row-major, NULL = zero */
                                       const double* dx,    /* r, NULL = state untouched */
                                       double* elapsed_ms); /* HIP-event time of the launch only (nullable) */

/* Measurement update and scoring for a Jacobian given by its non-zero columns: the Jacobian every landmark-SLAM caller
 * has.  The reference's Hj (ekf_slam.cpp:140-178) is non-zero in five columns, the pose columns 0, 1, 2 and the landmark
 * columns 3 + 2 i, 4 + 2 i.  H is the m x N matrix that is zero except H[:, cols[k]] = Hc[:, k], k = 0 .. s - 1;
 * ekf_dense64_correct_sparse is ekf_dense64_correct for that H and ekf_dense64_score_sparse is ekf_dense64_score for
 * those H_j, with the same operand order (T = H Sigma from rows of Sigma, U = Sigma H^T from columns, Sigma never
 * symmetrised), the same elimination, the same verdict rule and the same nullability of nu / nis_out / S_out / flag_out
 * and meaning of r_shared.  What changes is the cost: the panels of a correction are gathered from s rows and s columns
 * of Sigma (O(s N) bytes instead of a pass over Sigma; four launches instead of six, the last two -- gain and rank-m
 * update, 16 N^2 bytes -- being the dense call's own), and a score needs the s x s block Sigma[cols_j, cols_j] alone (one
 * launch, no pass over Sigma, candidates as [J][m][s] instead of [J][m][N]).
 * cols: distinct indices in [0, N) in any order (per candidate: [J][s], each row distinct); Hc: m x s row-major
 * ([J][m][s]); 1 <= m <= min(N, EKF_DENSE64_MAX_M), 1 <= s <= min(N, EKF_DENSE64_MAX_S), m > s is allowed (R makes S
 * regular), J >= 1, J * m <= EKF_DENSE64_SCORE_SPARSE_MAX_ROWS -- the reference's data_association() scores a reading
 * against every known landmark (:300-314), 5000 candidates at N = 10003, in one call.
 * A NULL handle (checked first), NULL cols / Hc / R, a bad m, s or J, a negative, out-of-range or repeated index in any
 * row of cols (checked on the host), nis_out without nu or, for the scoring, no output at all return EKF_ERR_INVALID
 * before the device is looked at.  A singular or non-finite S returns EKF_ERR_STATE from the correction and leaves state
 * and Sigma bit for bit (the verdict word is read before the first store); in the scoring it is flag 1 and nis = NaN for
 * that candidate only and the call returns EKF_OK.  The scoring is read-only.  The padding of Sigma and of the state
 * stays zero, so propagate_block / score_sparse / correct_sparse make a whole SLAM cycle without Sigma leaving the device
 * (INTEGRATION.md spells the reference's loop with them).
 * ORDER OF ARITHMETIC (part of the contract): every entry of T, of U and of S - R is a dot product of exactly s terms,
 * accumulated from +0 in ascending k of the list with one fused multiply-add per term:
 *   T[a][j] = sum_k Hc[a][k] Sigma[cols[k]][j]     U[i][a] = sum_k Sigma[i][cols[k]] Hc[a][k]
 *   S[a][b] = (sum_k T[a][cols[k]] Hc[b][k]) + R[a][b]      (the inner T rounded to fp64 first, R by one plain addition)
 * S, its elimination, nis and the flag come from one device routine that both entry points launch, and there are no
 * floating-point atomics.  So S, nis and flag of a candidate are the same bits alone or at any position of any batch,
 * with R shared or replicated, in score_sparse and in the correct_sparse that follows with the same operands, wherever
 * the listed columns sit in Sigma (in any N) given the same values of Sigma[cols, cols], and from run to run.  Permuting
 * cols together with the columns of Hc changes the order of the sums: the result agrees to rounding, not bit for bit;
 * nor is it bit-equal to the dense calls, which sum per-chunk partials.
 * Memory: the correction uses the operand buffer and workspace of ekf_dense64_correct; the scoring allocates one buffer
 * for its operands and results on first use (8 (J m s + J m m + ..) bytes, nothing of size ld^2), which grows with larger
 * calls; a failure there returns EKF_ERR_NOMEM and leaves the handle as it was.
 * Both are model-free (wrapping an angle is the caller's business) and synchronous, on the handle's stream.
 * elapsed_ms (nullable) = HIP-event time of the launches only. */
#define EKF_DENSE64_MAX_S 64                       /* listed columns of one Jacobian */
#define EKF_DENSE64_SCORE_SPARSE_MAX_ROWS 65536    /* J * m of one ekf_dense64_score_sparse call */
ekf_status ekf_dense64_correct_sparse(ekf_dense64_handle h, int m, int s,
                                      const int* cols,      /* [s] distinct column indices in [0, N) */
                                      const double* Hc,     /* m x s row-major: column k is H[:, cols[k]] */
                                      const double* R,      /* m x m */
                                      const double* nu,     /* m, NULL: state untouched, nis_out must be NULL */
                                      double* nis_out, double* elapsed_ms);
ekf_status ekf_dense64_score_sparse(ekf_dense64_handle h, int J, int m, int s,
                                    const int* cols,        /* [J][s], each row distinct */
                                    const double* Hc,       /* [J][m][s] */
                                    const double* R, int r_shared, const double* nu,
                                    double* nis_out, double* S_out, int* flag_out, double* elapsed_ms);

/* Deferred sparse corrections: one pass over Sigma per tick instead of one per reading.  ekf_dense64_correct_sparse ends in
 * the rank-m update Sigma <- Sigma - K T, which rewrites all of Sigma (16 N^2 bytes); a tick with V readings streams Sigma
 * V times.  The deferred form keeps the factors instead: the handle holds p <= EKF_DENSE64_PENDING_MAX_ROWS pending rows of
 * K and of T, the current covariance is
 *   Sigma_cur = Sigma_base - sum_{q < p} K^T[q] T[q]        (Sigma_base: what is in memory; never symmetrised)
 * and Sigma_base is rewritten once, by the flush (one launch of the rank-m update at rank p).  Nothing is approximated:
 * the deferred sequence is the eager one up to the rounding of another order of summation.
 * ekf_dense64_correct_sparse_deferred: the arguments, the argument checks (in the same order), the verdict rule and the
 *   one synchronisation of ekf_dense64_correct_sparse, and its results for Sigma_cur: S, nis, K, state += K nu at once
 *   (get_state* / set_state* are never stale and never flush).  Sigma in memory is not written; K (m rows) and
 *   T = Hc Sigma_cur[cols, :] (m rows) are appended to the pending panels.  With p + m > 64 it flushes first.  A singular
 *   or non-finite S returns EKF_ERR_STATE and leaves the state, Sigma and the pending rows bit for bit and their count as
 *   it was (a flush the call had to make first stands: it changes the representation, not Sigma_cur).
 * ekf_dense64_score_sparse with rows pending scores against Sigma_cur (with none it launches what it always did).
 * Every other entry point that reads or writes Sigma -- propagate, propagate_block, correct, score, correct_sparse,
 *   init_block, get_sigma, get_sigma_block -- flushes first when rows are pending, after its own argument checks (a
 *   refused call changes nothing, the pending rows included) and inside its elapsed_ms; with nothing pending none of them
 *   does anything new.  ekf_dense64_set with a Sigma drops the pending rows (they belonged to the covariance it replaces),
 *   with F or Q alone it leaves them; destroy drops them.
 * ekf_dense64_flush: Sigma_base <- Sigma_cur now; with nothing pending a no-op that reports 0 ms without looking at the
 *   device.  ekf_dense64_pending: the rows waiting, 0 .. 64.
 * ORDER OF ARITHMETIC (part of the contract): wherever the sparse calls read an entry of Sigma, the deferred ones read
 *   x = Sigma_base[i][j];  x = fma(-K^T[q][i], T[q][j], x)  for q = 0, 1, .. p - 1
 * one fused multiply-add per pending row in ascending q, and then run the sparse calls' own dot products on x.  No
 * floating-point atomics.  So S, nis and flag of a candidate are the same bits alone or at any position of any batch, in
 * score_sparse and in the deferred correction that follows with the same operands, and from run to run, with rows pending
 * too.  The flush sums its p terms in the order of v_mfma_f64_16x16x4_f64, so a deferred sequence agrees with the eager one
 * to rounding, not in bits -- except that with nothing pending ONE deferred correction followed by the flush runs the
 * arithmetic of ekf_dense64_correct_sparse on the same operands and is bit-identical to it (state, Sigma, nis).
 * Memory: the pending panels, 2 * 64 * ld doubles (10.4 MB at N = 10003), are allocated by the first deferred call; a
 * failure there returns EKF_ERR_NOMEM and leaves the handle as it was.  elapsed_ms (nullable) = HIP-event time of the
 * launches only. */
#define EKF_DENSE64_PENDING_MAX_ROWS 64
ekf_status ekf_dense64_correct_sparse_deferred(ekf_dense64_handle h, int m, int s, const int* cols, const double* Hc,
                                               const double* R, const double* nu, double* nis_out, double* elapsed_ms);
ekf_status ekf_dense64_flush(ekf_dense64_handle h, double* elapsed_ms);    /* no-op, 0 ms, with nothing pending */
ekf_status ekf_dense64_pending(ekf_dense64_handle h, int* rows);           /* rows of K / T waiting, 0 .. 64 */

/* The Joseph form of ekf_dense64_correct_sparse, with per-state gain weights.  The short form Sigma <- Sigma - K T is the
 * covariance of the updated state for the exact optimal gain only, and it cancels when a prior variance is large against
 * R.  The Joseph form
 *   Sigma <- (I - K H) Sigma (I - K H)^T + K R K^T  =  Sigma - K T - U K^T + K S K^T      (U = Sigma H^T, S = T H^T + R)
 * is a sum of congruences: it stays positive semi-definite up to rounding and it holds for ANY gain.  With D = U - K S, the
 * residual of the gain equation (zero up to rounding for the optimal gain), it is Sigma <- Sigma - K T - D K^T: one
 * read-modify-write pass of rank 2 m over Sigma.  "Any gain" is used for the PARTIAL UPDATE (Schmidt-Kalman): per-state
 * weights w in [0, 1] give K = diag(w) U S^-1; a state with w = 0 is a CONSIDER state, whose estimate and own covariance
 * block stay untouched while its cross-covariances stay consistent.
 * cols, Hc, R, nu, nis_out, the verdict rule and the order of the argument checks are ekf_dense64_correct_sparse's; only the
 * cap on m differs, 1 <= m <= EKF_DENSE64_JOSEPH_MAX_M (the two stacked panels of m rows fit the 64-row panel stride).
 * SAME T, U, S, S^-1, nis: they are the bits ekf_dense64_correct_sparse computes for the same arguments on the same Sigma
 *   (the same gather, sum and elimination code is launched).
 * THE GAIN: K[i][k] = +0.0 when w_i == 0, otherwise fl(w_i * G[i][k]), with G = U S^-1 summed as the short form's gain
 *   kernel sums it (l ascending, a product and an addition per term).  Rows i >= Na are zero.
 * THE STATE: state[i] += sum_k K[i][k] nu[k] in that kernel's fold (eight partial sums over k = g, g + 8, .., then g
 *   ascending).  A state with w_i == 0 is NOT WRITTEN.
 * THE RESIDUAL: D[i][k] = U[i][k] - sum_l K[i][l] S[l][k]: the accumulator starts at U[i][k] and takes one fused
 *   multiply-add per l, ascending.  S is the summed S, the matrix S_out of ekf_dense64_score_sparse returns.
 * THE COVARIANCE: Sigma[i][j] <- Sigma[i][j] - sum_k K[i][k] T[k][j] - sum_k D[i][k] K[j][k] for i, j < Na.  All 2 m
 *   products are folded into ONE accumulator that starts at Sigma[i][j]; the K T terms come first, then the D K^T terms.
 *   The association inside a group of terms is the implementation's (chains of v_mfma_f64_16x16x4_f64, four terms each); it
 *   depends on (m, tile shape) alone.  There are no atomics on floating-point data, and a run repeats bit for bit.
 * THE CONSIDER RULE (a definition, not only an optimisation): an entry Sigma[i][j] with w_i == 0 and w_j == 0 enters no
 *   result and is not written -- a NaN, an Inf or a -0.0 there keeps its bits.  An entry with w_i == 0 takes the D K^T terms
 *   only, with D[i] = U[i]; an entry with w_j == 0 takes the K T terms only.
 * TILES: the pass works on tiles of tile_rows x tile_cols entries (ekf_dense64_joseph_launch_info; aligned at 0).  A tile
 *   whose rows and columns are all considered is not touched, so the cost follows the active states even while they are
 *   still correlated with the rest (ekf_dense64_set_live needs a decoupled tail for that).  *tiles_skipped (nullable) is the
 *   number of untouched tiles, a pure function of (Na, w, tile shape): (row groups without a w != 0) * (column groups
 *   without one); 0 with gain_w == NULL.
 * gain_w: N doubles (the handle's N), NULL = all 1.  Every value among the first Na must be finite and in [0, 1], else the
 *   call returns EKF_ERR_INVALID before the device is looked at (a host scan, after the checks above); values at indices
 *   >= Na are ignored.
 * EAGER ONLY: the call needs Sigma in memory, so it FLUSHES THE PENDING ROWS FIRST, after its argument checks (a refused
 *   call leaves them in place) and inside the timed region, as ekf_dense64_health does.
 * LIVE: a structured call on the live corner.  Nothing at a row or column >= Na is read or written; accesses are masked
 *   element by element.
 * A singular or non-finite S returns EKF_ERR_STATE; Sigma and the state stay exactly as they were, except that the flush, if
 *   any, has happened.  The writing launches read the verdict word before their first store.
 * Four launches (gather, scoring with J = 1, gain, update), synchronous, on the handle's stream; it uses the operand buffer
 * and the workspace of ekf_dense64_correct and allocates nothing.  elapsed_ms (nullable) = HIP-event time of the launches. */
#define EKF_DENSE64_JOSEPH_MAX_M 32
ekf_status ekf_dense64_correct_sparse_joseph(ekf_dense64_handle h, int m, int s, const int* cols, const double* Hc,
                                             const double* R, const double* nu,
                                             const double* gain_w /* N doubles (the handle's N), NULL = all 1 */,
                                             double* nis_out, long long* tiles_skipped /* nullable */,
                                             double* elapsed_ms);
ekf_status ekf_dense64_joseph_launch_info(ekf_dense64_handle h, int* tile_rows, int* tile_cols, int* threads);

/* The landmark front end: the reference's data_association() (ekf_slam.cpp:278-402) on the handle's own state.  The sparse
 * calls above are model-free, so a caller that spells the reference's loop with them reads the state back,
 * builds one Jacobian per known landmark on the host, sends them up, takes the scores down, decides, and builds the
 * winner's operands again -- five or six synchronous calls around one scoring launch.  Everything in between is a function
 * of values that already sit in device memory; these two calls keep it there.  They are a layer over the calls above and
 * below (score_sparse, correct_sparse[_deferred], init_block, set_live), which stay exactly as they are.
 * State layout: [theta, x, y, m1x, m1y, ...], landmark i at 3 + 2 i, 4 + 2 i.  params: sigma0_landmark, r_meas, gate_new,
 * gate_update are used; NULL = the reference's constants (ekf_default_params).
 * OPERANDS, built on the device by one thread per candidate from the device helpers of the single-filter path (the same
 * source, compiled with the library's -ffp-contract=off): candidate i has cols = {0, 1, 2, 3 + 2 i, 4 + 2 i}; Hc is the
 * reference's Hj at those columns (:158-166: four divisions and one sqrt); R = r_meas I, shared; nu = z - zhat with
 * z = (sqrt(sx^2 + sy^2), atan2(sy, sx)) and the predicted bearing wrapped (:152-155).  The innovation itself is RAW for
 * scoring -- the reference's own quirk (:269) -- and WRAPPED in its bearing for the correction (:183).
 * ekf_dense64_score_landmarks: calculate_maha_dis (:217-276) of one reading against landmarks [first_lm, first_lm + count).
 *   It is ekf_dense64_score_sparse(J = count, m = 2, s = 5, r_shared = 1) on those operands: the same kernel (eager, or
 *   read-through as rows are pending), the same flags (flag 1 and nis = NaN for a singular or non-finite S), the same
 *   nullability (nis_out, S_out, flag_out not all NULL).  nis, S and flag are bit for bit what ekf_dense64_score_sparse
 *   returns when it is handed cols_out, Hc_out, nu_out back.  1 <= count <= EKF_DENSE64_SCORE_SPARSE_MAX_ROWS / 2,
 *   first_lm >= 0, 3 + 2 (first_lm + count) <= live; otherwise EKF_ERR_INVALID before the device is looked at, a NULL
 *   handle first.  Read-only: Sigma, the state and the pending rows are untouched.  One synchronisation; nothing goes up.
 * ekf_dense64_associate_landmarks: data_association for J readings in order.  *known (IN/OUT) counts the initialised
 *   landmarks, which are landmarks 0 .. *known - 1; n_max is the map's capacity.  Per reading, THE RULE (:293-330):
 *     best = gate_new, win = known; the known landmarks are scored (as above) and visited in ascending index with a strict
 *     <, so the first of equal scores wins; a NaN score -- a flagged candidate -- never wins and disturbs nobody else.
 *     win == known and known < n_max: a new landmark.  Its state becomes initialize_landmark's position (:200-214), its
 *       covariance goes through ekf_dense64_init_block's path with s = 0 and W = sigma0_landmark I, *known is incremented,
 *       and the gate below sees best = 0.
 *     best < gate_update: the winner's operands are rebuilt from the current state (after an initialisation) and the
 *       correction runs -- ekf_dense64_correct_sparse, or ekf_dense64_correct_sparse_deferred with
 *       EKF_DENSE64_LM_DEFERRED -- and then state[0] = normalize_angle(state[0]) is stored unconditionally, as :187 / :385
 *       do (a heading of -0.0 becomes +0.0, as in the reference).
 *     otherwise the reading is dropped and nothing at all is written; known == n_max with nothing under gate_new drops it.
 *   assoc_out[j] (nullable): the landmark corrected, -1 for a reading that was dropped (or whose correction was refused, or
 *   that initialised a landmark without correcting it, which only a gate_update <= 0 does), -2 for a reading the call did
 *   not reach.  best_out[j] (nullable): the winning score, gate_new when no known landmark won (a new landmark included).
 *   COMPOSITION: the call goes through the internal paths of the calls it names, so every rule of theirs holds unchanged:
 *   scores read through the pending rows, a deferred correction flushes first when its two rows do not fit, the eager one
 *   and init_block flush first -- or, with the carry policy on, init_block maps the pending rows.  For one reading the
 *   state and Sigma afterwards are bit for bit those of a twin handle on which the host makes the same decision and calls
 *   init_block (W, xb) / correct_sparse[_deferred] with the operands the device built, and sets the heading.
 *   EKF_DENSE64_LM_GROW_LIVE: a new landmark first grows the live dimension to 3 + 2 (known + 1) when it is smaller, by
 *   ekf_dense64_set_live (exact, keeps the pending rows).  Without it a new landmark beyond the live dimension returns
 *   EKF_ERR_INVALID before that reading changes anything; earlier readings stand.
 *   FAILURES: checked before the device is looked at, in this order: NULL handle; NULL known or meas_xy; J < 1; n_max < 0
 *   or 3 + 2 n_max > N; *known outside [0, n_max]; 3 + 2 *known > live; unknown flag bits -> EKF_ERR_INVALID, nothing
 *   changes.  A singular or non-finite S of the winner returns EKF_ERR_STATE from that reading's correction, with that
 *   reading's effects as the sparse calls define them (state, Sigma and pending rows as before the correction; an
 *   initialisation that preceded it stands and is counted in *known; the heading is not rewritten).  Earlier readings
 *   stand, later assoc_out entries are -2, *known is what it was after the last completed step.
 *   SYNCHRONISATION: two points per reading -- the 32-byte decision record {win, kind, best, runner-up}, and the
 *   correction's own (a dropped reading has the first only).  One case has a third: a new landmark that grows the live
 *   dimension (EKF_DENSE64_LM_GROW_LIVE) while rows are pending goes through ekf_dense64_set_live, which clears the new
 *   columns of the pending panels and synchronises; with nothing pending the growth costs nothing.  A reading goes up as sixteen bytes of kernel arguments; no
 *   candidate array goes up and no state comes down.  No floating-point atomics; the decision does not depend on the launch
 *   geometry (ties resolve to the lower index at every level of the reduction): the same inputs give the same bits on every
 *   run.  Memory: the scoring buffer of ekf_dense64_score_sparse, reserved once per call for n_max candidates (so a map
 *   that is being discovered never reallocates it), the pending panels with EKF_DENSE64_LM_DEFERRED, 32 bytes
 *   for the record; a failure to reserve returns EKF_ERR_NOMEM / EKF_ERR_HIP and leaves the handle as it was.
 * elapsed_ms (nullable) = HIP-event time of the launches only, summed over the readings, those of a reading that ends in
 * EKF_ERR_STATE or in the live refusal included. */
ekf_status ekf_dense64_score_landmarks(ekf_dense64_handle h, const ekf_params* params,
                                       double sx, double sy, int first_lm, int count,
                                       double* nis_out,   /* [count]            nullable */
                                       double* S_out,     /* [count][2][2]      nullable */
                                       int* flag_out,     /* [count]            nullable */
                                       int* cols_out,     /* [count][5]         nullable: the operands the device built */
                                       double* Hc_out,    /* [count][2][5]      nullable */
                                       double* nu_out,    /* [count][2] raw (un-wrapped) innovation, nullable */
                                       double* elapsed_ms);
#define EKF_DENSE64_LM_DEFERRED  1u  /* corrections through the deferred path (pending rows), else correct_sparse */
#define EKF_DENSE64_LM_GROW_LIVE 2u  /* a new landmark first grows the live dimension to 3 + 2 (known + 1) if it is smaller */
/* EKF_DENSE64_LM_JOSEPH (ekf_dense64_measure_landmarks, ekf_dense64_associate_landmarks, ekf_dense64_merge_landmarks; every
 * other call refuses it as an unknown bit): the call's corrections go through ekf_dense64_correct_sparse_joseph's internal
 * path with gain_w = NULL instead of ekf_dense64_correct_sparse's.  An eager form: together with EKF_DENSE64_LM_DEFERRED the
 * call returns EKF_ERR_INVALID where it checks its flag bits.  Without the flag every launch and every bit is as before. */
#define EKF_DENSE64_LM_JOSEPH    8u  /* corrections in the Joseph form (eager only); 4u stays an unknown bit */
ekf_status ekf_dense64_associate_landmarks(ekf_dense64_handle h, const ekf_params* params, int J,
                                           const double* meas_xy /* [J][2] */, int n_max, int* known /* IN/OUT */,
                                           unsigned flags,
                                           int* assoc_out,    /* [J] landmark corrected, -1 dropped, -2 not reached; nullable */
                                           double* best_out,  /* [J] winning score (gate_new when nothing won); nullable */
                                           double* elapsed_ms);

/* A laser scan as the handle's input.  What the reference's robot produces is a LaserScan of 360 ranges; it goes through
 * nuslam/src/landmarks.cpp:141 and CircleFitting::approxCirclePositions (circle_fitting.cpp:11-304) and reaches
 * data_association() as a list of circle centres (unknown_data_assoc.cpp:309-320, :414-415).  ekf_circle_fit_scans does that
 * for thousands of scans at once, bound to no handle and no stream, with six allocations per call and a kernel that gives a
 * cluster one lane.  These two calls do it for ONE scan on the handle's own device and stream.
 * THE KERNEL (k_scan_circles) is one workgroup of four waves: every beam computes its own cluster boundary, starts, lengths
 * and numbers come from ballot words and bit counts (clusters numbered in ascending beam order), the wrap merge follows, and
 * each cluster is fitted by one WAVE with its points spread over the lanes.  Every quirk of the reference that
 * ekf_circle_fit_scans keeps is kept: the `i != nb-1` boundary (the last beam always closes a cluster and belongs to none),
 * "more than 6 points", the merge of the last cluster into the first when their end points are within 0.2, a lone cluster
 * that merges with itself and vanishes, a scan without a cluster giving 0 circles (undefined in the reference), the
 * sv[3] < 1e-12 branch, "smallest positive eigenvalue, start 1000", the classification 1.5708 < mean_angle < 2.3562 &&
 * rad < 0.2, circles kept in cluster order up to max_out; at most 128 clusters, the first ones in beam order.
 * NUMBERS: the sums run in another order than ekf_circle_fit_scans' and LAPACK's, so nothing is bit-identical to either; the
 * contract is the one ekf_circle_fit_scans is held to against the checker: the same clusters, the same classification,
 * kept circles within 1e-9 in centre and radius, the others within 1e-6 relative.  POSITION INDEPENDENCE: every sum over a
 * cluster's points is a per-lane partial over k = lane, lane + 64, .. followed by a fixed butterfly, so a cluster's row of
 * all_clusters is a function of its points alone, bit for bit -- not of the wave that fitted it, of its number, or of what
 * else the scan holds.  No atomics; the same scan gives the same bits on every run.
 * ekf_dense64_fit_scan: ranges [n_beams] go up through a ring of pinned buffers, one launch, and the record {*count_out,
 *   *n_clusters, centres, radii} comes down in one copy behind ONE synchronisation; all_clusters ([128][4] = x, y, r,
 *   is_circle of every cluster, nullable) comes in the same synchronisation when asked for.  centres_out [max_out][2] and
 *   radii_out [max_out] (nullable) are zero beyond *count_out, all_clusters beyond *n_clusters.  READ-ONLY with respect to
 *   the filter: the state, Sigma and the pending rows are untouched in bits, nothing is flushed.
 *   1 <= n_beams <= EKF_DENSE64_SCAN_MAX_BEAMS, 1 <= max_out <= EKF_DENSE64_SCAN_MAX_CIRCLES.  Memory: one device buffer of
 *   15.2 KB and the ring (8 x 8 KB pinned), reserved by the first call and reused; no later call allocates.
 * ekf_dense64_associate_scan: ekf_dense64_fit_scan(max_out = max_readings) followed by exactly the per-reading path of
 *   ekf_dense64_associate_landmarks on the first *count_out = min(circles, max_readings) centres in cluster order: THE RULE,
 *   COMPOSITION, both flags, the failure semantics and the two synchronisations per reading of that call hold unchanged,
 *   and the state, Sigma, the pending rows, *known, assoc_out and best_out afterwards are bit for bit those of a twin
 *   handle on which ekf_dense64_fit_scan and ekf_dense64_associate_landmarks(J = count, centres) are called.  A scan
 *   without a circle returns EKF_OK with *count_out = 0 after the fit's one synchronisation; nothing of the filter is
 *   written.  centres_out [max_readings][2] (nullable): the readings, zero beyond the count; assoc_out [max_readings]
 *   (nullable): as there, -2 beyond the count; best_out [max_readings] (nullable): gate_new beyond it.
 * FAILURES, checked before the device is looked at, in this order: NULL handle; NULL ranges or count_out (or known);
 * n_beams, max_out / max_readings out of range; then, for associate_scan, the checks of ekf_dense64_associate_landmarks in
 * its order (n_max, *known, the live dimension, flag bits) -> EKF_ERR_INVALID, nothing changes.
 * elapsed_ms (nullable) = HIP-event time of the launches: the circle kernel, plus the readings' as there. */
#define EKF_DENSE64_SCAN_MAX_BEAMS 1024
#define EKF_DENSE64_SCAN_MAX_CIRCLES 128
ekf_status ekf_dense64_fit_scan(ekf_dense64_handle h, const double* ranges /* [n_beams] */, int n_beams, int max_out,
                                int* count_out, double* centres_out /* [max_out][2] nullable */,
                                double* radii_out /* [max_out] nullable */,
                                double* all_clusters /* [128][4] nullable */, int* n_clusters /* nullable */,
                                double* elapsed_ms);
ekf_status ekf_dense64_associate_scan(ekf_dense64_handle h, const ekf_params* params,
                                      const double* ranges /* [n_beams] */, int n_beams, int max_readings,
                                      int n_max, int* known /* IN/OUT */, unsigned flags,
                                      int* count_out, double* centres_out /* [max_readings][2] nullable */,
                                      int* assoc_out /* [max_readings] nullable */,
                                      double* best_out /* [max_readings] nullable */, double* elapsed_ms);

/* A whole scan associated JOINTLY: the textbook alternative to the reading-by-reading rule above, and a new capability
 * beside it, not a faster form of it.  All J readings are scored against the state the scan was taken at (as the reference's
 * measurement() captures the pose once per call, :109-111), ONE assignment is made, and the matched and new readings are
 * corrected in stacked updates of dimension 2 V.  ekf_dense64_associate_landmarks pays two synchronisations, a scoring launch
 * over the map and (eager) a pass over Sigma PER READING; this call pays one decision synchronisation per scan and one pass
 * per 30 readings.  The results differ from the sequential rule's wherever a reading's correction would have moved a later
 * reading's scores; with J = 1 the two calls coincide bit for bit (state, Sigma, pending rows, assoc_out, best_out).
 * ekf_dense64_score_readings: read-only.  Candidate (j, i) is reading j against landmark first_lm + i; nis_out and flag_out
 *   [J][count] (nullable, not both NULL) are bit for bit what ekf_dense64_score_landmarks returns for reading j alone: the
 *   same model source, the same scoring kernel, read-through with rows pending.  The readings go up once in one copy, they
 *   are cut into launches of at most 32768 / count readings (a launch stays within EKF_DENSE64_SCORE_SPARSE_MAX_ROWS), and
 *   the outputs come down behind ONE synchronisation.  1 <= J <= EKF_DENSE64_JOINT_MAX_READINGS, 1 <= count <= 32768,
 *   first_lm >= 0, 3 + 2 (first_lm + count) <= live; otherwise EKF_ERR_INVALID before the device is looked at.
 * ekf_dense64_joint_operands: a read-only hook, the stacked operands the joint correction would use for V pairs (landmark
 *   lm_idx[v], reading v), built from the CURRENT state: cols = {0, 1, 2, 3 + 2 i0, 4 + 2 i0, 3 + 2 i1, ..}; Hc [2V][3 + 2V]
 *   is zero except that rows 2v and 2v + 1 hold the reference's Hj (:158-166) at the local columns 0 .. 2 and 3 + 2v, 4 + 2v;
 *   nu [2V] has its bearing wrapped (:183); R = r_meas I is implied and not returned.  At V = 1 these are the operands of
 *   ekf_dense64_score_landmarks with the bearing wrapped.  1 <= V <= EKF_DENSE64_JOINT_MAX_PAIRS, the landmarks distinct
 *   and inside the live dimension, the outputs nullable but not all NULL; otherwise EKF_ERR_INVALID.
 * ekf_dense64_associate_joint, THE JOINT RULE:
 *   1 SCORE: all J readings against landmarks 0 .. *known - 1 at the state on entry, as ekf_dense64_score_readings does.
 *   2 PER READING: best = gate_new, win = known, the lexicographic (score, index) minimum with NaNs skipped, as THE RULE
 *     above.  MATCH when win < known and best < gate_update; NEW when win == known; otherwise DROP.
 *   3 RESOLVE: of the MATCH readings that claim one landmark the smallest (best, j) keeps it and the others become DROP.
 *     The NEW readings take the slots known, known + 1, .. in ascending j while slot < n_max; beyond that they become DROP.
 *     TWO READINGS CLASSED NEW IN ONE CALL GIVE TWO LANDMARKS, also when they see the same object: nothing is scored
 *     against a landmark that does not exist yet.  ekf_dense64_score_landmark_pairs / ekf_dense64_merge_landmarks is the
 *     repair.  The records, the counts and the new landmarks' positions (initialize_landmark, :200-214, at the pose on
 *     entry) come down in one copy behind the FIRST synchronisation; best_out[j] is filled from it.
 *   4 LIVE: checked once, 3 + 2 (known + n_new) <= live.  EKF_DENSE64_LM_GROW_LIVE grows it by one ekf_dense64_set_live;
 *     without the flag the call returns EKF_ERR_INVALID and nothing at all has been written.
 *   5 INIT: the new landmarks in groups of at most 32, each ONE pass through ekf_dense64_init_block's path with first =
 *     3 + 2 slot, r = 2 n, s = 0, W = sigma0_landmark I and the stacked positions -- bit for bit n calls with r = 2; carry
 *     and pending rows as that call defines.  *known grows by the number initialised.
 *   6 CORRECT: the pairs are the MATCH and NEW readings with their landmarks in ascending j (MATCH only with gate_update
 *     <= 0, as in the sequential call), cut greedily into groups of at most EKF_DENSE64_JOINT_MAX_PAIRS.  Per group the
 *     operands of ekf_dense64_joint_operands are built from the THEN-CURRENT state, ekf_dense64_correct_sparse (or
 *     _deferred with EKF_DENSE64_LM_DEFERRED) runs through its internal path at m = 2 V, s = 3 + 2 V, and the heading is
 *     normalised and stored.  Each group has the correction's own synchronisation.
 *   assoc_out[j] (nullable): the landmark corrected; -1 for a dropped reading, one that lost a conflict, one that
 *   initialised a landmark without correcting it, or one of a refused group; -2 for a reading of a group that was not
 *   reached.  best_out[j] (nullable) as above.  n_groups_out (nullable): the number of groups the pairs were cut into.
 *   TWIN CONTRACT: the state, Sigma, the pending rows and *known afterwards are bit for bit those of a twin handle on which
 *   the host calls ekf_dense64_score_landmarks per reading, applies the rule, calls ekf_dense64_init_block per group, then
 *   per group ekf_dense64_joint_operands followed by ekf_dense64_correct_sparse[_deferred] with what it returned and
 *   R = r_meas I, and sets the heading.
 *   FAILURES, checked before the device is looked at, in this order: NULL handle; NULL known or meas_xy; J outside [1,
 *   EKF_DENSE64_JOINT_MAX_READINGS]; then the checks of ekf_dense64_associate_landmarks unchanged (n_max, *known, the live
 *   dimension, flag bits); n_max > 32768 -> EKF_ERR_INVALID, nothing changes.  A singular or non-finite S of a group
 *   returns EKF_ERR_STATE with that group's correction undone as the sparse calls define; earlier groups and the
 *   initialisations stand, *known is what it was after the initialisations.
 *   No floating-point atomics and no in-kernel waits; every reduction resolves ties to the lower index, so the same inputs
 *   give the same bits on every run.  Memory: 78 KB for the call's own buffer, the scoring buffer reserved once per call for
 *   min(J, 32768 / n_max) n_max candidates, the pending panels with EKF_DENSE64_LM_DEFERRED.
 * ekf_dense64_associate_scan_joint: ekf_dense64_fit_scan(max_out = max_readings) followed by the same path on the centres,
 *   exactly as ekf_dense64_associate_scan wraps the sequential loop; its checks first, in that call's order.
 * elapsed_ms (nullable) = HIP-event time of the launches, summed over the call's synchronisations. */
#define EKF_DENSE64_JOINT_MAX_READINGS 128   /* = EKF_DENSE64_SCAN_MAX_CIRCLES */
#define EKF_DENSE64_JOINT_MAX_PAIRS     30   /* m = 2V <= 64 and s = 3 + 2V <= 64 */
ekf_status ekf_dense64_score_readings(ekf_dense64_handle h, const ekf_params* params, int J,
                                      const double* meas_xy /* [J][2] */, int first_lm, int count,
                                      double* nis_out /* [J][count] nullable */, int* flag_out /* [J][count] nullable */,
                                      double* elapsed_ms);
ekf_status ekf_dense64_joint_operands(ekf_dense64_handle h, const ekf_params* params, int V,
                                      const int* lm_idx /* [V] */, const double* meas_xy /* [V][2] */,
                                      int* cols_out /* [3 + 2V] nullable */, double* Hc_out /* [2V][3 + 2V] nullable */,
                                      double* nu_out /* [2V] bearing wrapped, nullable */, double* elapsed_ms);
ekf_status ekf_dense64_associate_joint(ekf_dense64_handle h, const ekf_params* params, int J,
                                       const double* meas_xy /* [J][2] */, int n_max, int* known /* IN/OUT */,
                                       unsigned flags, int* assoc_out /* [J] nullable */,
                                       double* best_out /* [J] nullable */, int* n_groups_out /* nullable */,
                                       double* elapsed_ms);
ekf_status ekf_dense64_associate_scan_joint(ekf_dense64_handle h, const ekf_params* params,
                                            const double* ranges /* [n_beams] */, int n_beams, int max_readings,
                                            int n_max, int* known /* IN/OUT */, unsigned flags,
                                            int* count_out, double* centres_out /* [max_readings][2] nullable */,
                                            int* assoc_out /* [max_readings] nullable */,
                                            double* best_out /* [max_readings] nullable */, double* elapsed_ms);

/* JOINT COMPATIBILITY (JCBB, Neira & Tardos 2001) for a scan.  Both rules above are nearest neighbour: they decide per
 * reading and never look at the correlation between pairings.  With a pose error common to all readings and a map that is
 * tight in relative terms, a reading is individually compatible with its neighbour's landmark, and the per-reading argmin
 * pairs it there or loses a conflict and drops it.  The joint rule accepts the LARGEST set of pairings whose stacked
 * innovation passes ONE gate against its joint covariance S_H = H_H Sigma H_H^T + R.
 * THE DEVICE HALF is whatever touches Sigma: the scores (as ekf_dense64_score_readings), the candidates of each reading, their
 * operands, and the cross blocks between different candidate pairings, which no other call produces.
 *   CANDIDATES of reading j: the up to max_cand lowest (score, index) pairs with score < gate_ic in ascending lexicographic
 *   order; a NaN is never a candidate, ties go to the lower index, a score equal to gate_ic is not one.  best[j]: the overall
 *   minimum, gate_new when nothing lies below it; is_new[j] = (no landmark has score < gate_new).  The P candidates of a call
 *   are numbered in ascending (j, rank).
 *   W [2P][2P], row-major in candidate order; its 2 x 2 block (p, q) is, with cols_p = {0, 1, 2, 3 + 2 i_p, 4 + 2 i_p} and
 *   Hc_p, nu_p the operands of ekf_dense64_score_landmarks (bearing RAW),
 *     G[k][b]  = Sigma[cols_p[k]][cols_q[b]]                 (Sigma as stored, never symmetrised)
 *     T'[a][b] = sum_k fma(Hc_p[a][k], G[k][b], .)           from +0, k ascending, rounded to fp64
 *     W[a][b]  = sum_k fma(T'[a][k], Hc_q[b][k], .)          from +0, k ascending;  p == q: + r_meas delta_ab by one plain addition
 *   the order of the sparse scoring kernel: the diagonal block (p, p) is bit for bit the S_out of ekf_dense64_score_landmarks
 *   for that reading and landmark.  Blocks (p, q) and (q, p)^T may differ in bits, as Sigma[i][j] and Sigma[j][i] do.  A
 *   block's bits depend on its two candidates alone.  No atomics; the same inputs give the same bits on every run.
 * THE HOST HALF is the search (sequential, O(k^2) per node, on at most 512 KB).  Depth first over the readings in ascending
 *   j; at reading j its candidates in ascending rank, skipping a landmark the hypothesis uses already, then the branch "j
 *   unpaired".  An extension to k pairings is accepted only when its joint d2 < gate_joint[k - 1].  The incumbent starts as
 *   "nothing paired"; better means more pairings, then a smaller d2, then found first.  A node is pruned when pairings so far
 *   + readings still to come that have a candidate < the incumbent's pairings.  d2 comes from an incremental Cholesky factor
 *   along the path (pair number m owns rows 2m, 2m + 1; the block (new pair, earlier pair) = W[p_new][p_old], the lower
 *   triangle only): per new row r, columns c ascending, every product rounded and subtracted in turn, t ascending,
 *     v = W[r][c];  v = v - L[r][t] L[c][t] (t < c);  L[r][c] = v / L[c][c]
 *     d = W[r][r];  d = d - L[r][t]^2 (t < r);  not (finite and > 0): the extension is incompatible;  L[r][r] = sqrt(d)
 *     s = nu[r];  s = s - L[r][t] z[t] (t < r);  z[r] = s / L[r][r];  d2 = d2 + z[r]^2
 *   (the library is built with -ffp-contract=off; this order is part of the contract).  Every visit of a (reading, hypothesis)
 *   is one node; after max_nodes nodes the incumbent stands and exhausted = 1.  A function of its inputs.
 * ekf_dense64_jcbb_candidates: the read-only hook for the device half.  Pending rows are applied first (inside elapsed_ms,
 *   behind the argument checks) so that the scores, the selection and W see one Sigma in memory; nothing else is written.
 *   [terms | score | select] per scoring launch, [candidate terms | cross blocks], ONE synchronisation.  cand_lm_out and
 *   cand_nis_out are [J][max_cand] (-1 and +inf beyond cand_count_out[j]; cand_nis bit for bit ekf_dense64_score_readings');
 *   W_out must hold (2 min(J max_cand, 128))^2 doubles and receives [2P][2P] at the call's own P; nu_out [P][2].  Every
 *   output is nullable, not all.  1 <= J <= 32, 0 <= known <= 32768 inside the live dimension, gate_ic finite in (0,
 *   gate_new], 1 <= max_cand <= 4; otherwise EKF_ERR_INVALID before the device is looked at.
 * ekf_dense64_jcbb_search: the search as it stands; no handle, no device.  reading_of [P] ascending, lm_of [P], nis [P] (the
 *   caller's record: no decision reads it; nullable), W [2P][2P], nu [2P], gate_joint [J]; assign_out [J]: the candidate number
 *   of each reading or -1.  report: n_cand = P, n_pairs, n_drop = J - n_pairs, n_new = 0, exhausted, nodes, d2.
 * ekf_dense64_associate_jcbb, the whole rule:
 *   1 pending rows are applied.  2 SCORE as step 1 of THE JOINT RULE.  3 candidates (max_cand = 4) and cross blocks, ONE
 *   synchronisation, the search.  A reading of the chosen hypothesis is MATCH with its landmark; an unpaired reading with
 *   is_new is NEW and takes a slot in ascending j while slot < n_max, exactly as step 3 of THE JOINT RULE hands them out
 *   (the same kernel does it); every other reading is DROP.  Then steps 4 LIVE, 5 INIT and 6 CORRECT of THE JOINT RULE run
 *   unchanged, through the same internal functions: the corrections use the WRAPPED bearing and the operands of
 *   ekf_dense64_joint_operands from the then-current state.  The flags mean what they mean there.
 *   gate_joint NULL: gate_joint[k - 1] = k gate_ic.  *known = 0: nothing is scored, every reading is NEW.
 *   report: n_cand = P, n_pairs = the pairings of the hypothesis, n_new = the readings that got a slot, n_drop the rest.
 *   TWIN CONTRACT: the state, Sigma, the pending rows and *known afterwards are bit for bit those of a twin handle on which
 *   the host calls ekf_dense64_jcbb_candidates (max_cand = 4), ekf_dense64_jcbb_search, ekf_dense64_init_block per group,
 *   then per group ekf_dense64_joint_operands and ekf_dense64_correct_sparse[_deferred], and sets the heading.
 *   J = 1: the decision can differ from ekf_dense64_associate_joint's in the last bits of d2 (a Cholesky factor here, the
 *   Gauss-Jordan elimination of the scoring kernel there, and gate_ic in place of gate_update); not claimed bit-equal.
 *   FAILURES, checked before the device is looked at, in this order: NULL handle; NULL known or meas_xy; J outside [1, 32];
 *   the checks of ekf_dense64_associate_landmarks in its order; n_max > 32768; gate_ic not finite, <= 0 or > gate_new; a
 *   gate_joint entry not finite or <= 0; max_nodes outside [1, EKF_DENSE64_JCBB_MAX_NODES] -> EKF_ERR_INVALID, nothing changes.
 *   Memory: one buffer of 18 KB of operands plus 512 KB of W, reserved by the first call for the maxima; besides it what
 *   ekf_dense64_associate_joint reserves.  A failure returns EKF_ERR_NOMEM / EKF_ERR_HIP and leaves the handle as it was.
 * ekf_dense64_associate_scan_jcbb: ekf_dense64_fit_scan(max_out = max_readings <= 32) in front, as
 *   ekf_dense64_associate_scan_joint wraps the per-reading joint rule; gate_joint [max_readings] or NULL.
 * ekf_dense64_jcbb_launch_info: the cross kernel's tile (blocks per side) and threads per workgroup. */
#define EKF_DENSE64_JCBB_MAX_READINGS 32
#define EKF_DENSE64_JCBB_MAX_CAND      4          /* P <= 128, W <= 256 x 256 */
#define EKF_DENSE64_JCBB_MAX_NODES    (1 << 22)
typedef struct { int n_cand, n_pairs, n_new, n_drop, exhausted; long long nodes; double d2; } ekf_dense64_jcbb_report;
ekf_status ekf_dense64_jcbb_launch_info(ekf_dense64_handle h, int* tile, int* threads);
ekf_status ekf_dense64_jcbb_candidates(ekf_dense64_handle h, const ekf_params* params, int J,
                                       const double* meas_xy /* [J][2] */, int known, double gate_ic, int max_cand,
                                       int* cand_count_out /* [J] */, int* cand_lm_out /* [J][max_cand] */,
                                       double* cand_nis_out /* [J][max_cand] */, double* best_out /* [J] */,
                                       int* is_new_out /* [J] */, int* P_out, double* W_out /* [2P][2P] */,
                                       double* nu_out /* [P][2] raw */, double* elapsed_ms);
ekf_status ekf_dense64_jcbb_search(int J, int P, const int* reading_of /* [P] */, const int* lm_of /* [P] */,
                                   const double* nis /* [P] nullable */, const double* W /* [2P][2P] */,
                                   const double* nu /* [2P] */, const double* gate_joint /* [J] */, long long max_nodes,
                                   int* assign_out /* [J] */, ekf_dense64_jcbb_report* report /* nullable */);
ekf_status ekf_dense64_associate_jcbb(ekf_dense64_handle h, const ekf_params* params, int J,
                                      const double* meas_xy /* [J][2] */, int n_max, int* known /* IN/OUT */,
                                      double gate_ic, const double* gate_joint /* [J] nullable */, long long max_nodes,
                                      unsigned flags, int* assoc_out /* [J] nullable */, double* best_out /* [J] nullable */,
                                      ekf_dense64_jcbb_report* report /* nullable */, int* n_groups_out /* nullable */,
                                      double* elapsed_ms);
ekf_status ekf_dense64_associate_scan_jcbb(ekf_dense64_handle h, const ekf_params* params,
                                           const double* ranges /* [n_beams] */, int n_beams, int max_readings,
                                           int n_max, int* known /* IN/OUT */, double gate_ic,
                                           const double* gate_joint /* [max_readings] nullable */, long long max_nodes,
                                           unsigned flags, int* count_out,
                                           double* centres_out /* [max_readings][2] nullable */,
                                           int* assoc_out /* [max_readings] nullable */,
                                           double* best_out /* [max_readings] nullable */,
                                           ekf_dense64_jcbb_report* report /* nullable */, double* elapsed_ms);

/* The other two methods of rigid2d::EKF_SLAM on the handle's own state: prediction() (ekf_slam.cpp:55-106) and measurement()
 * (:108-197).  After ekf_dense64_associate_landmarks the heading lives on the device only -- it is corrected there and
 * nothing is read back -- so a caller of the model-free ekf_dense64_propagate_block would fetch state[0], evaluate four
 * transcendentals and upload three operands per tick.  These two calls keep that on the device as well; with them both
 * loops of the reference's nodes (slam: prediction + measurement; unknown_data_assoc: prediction + data_association) run
 * without the state leaving the device.  Layers over propagate_block and correct_sparse[_deferred], which stay as they are.
 * params: q_pose and straight_eps (prediction), r_meas (measurement) are used; NULL = the reference's constants.
 * ekf_dense64_predict_landmarks: prediction(Twist2D(dtheta, dx, 0)).
 *   OPERANDS, built by one thread on the device (the library's -ffp-contract=off) from theta = state[0]:
 *     |dtheta| < straight_eps (strict):  update = (0, dx cos(theta), dx sin(theta));  A(1,0) = -dx sin(theta),
 *       A(2,0) = dx cos(theta)                                                                          (:80-86)
 *     otherwise:  update = (dtheta, -(dx/dtheta) sin(theta) + (dx/dtheta) sin(theta + dtheta),
 *       (dx/dtheta) cos(theta) - (dx/dtheta) cos(theta + dtheta));  A(1,0) = -(dx/dtheta) cos(theta) + (dx/dtheta)
 *       cos(theta + dtheta), A(2,0) = -(dx/dtheta) sin(theta) + (dx/dtheta) sin(theta + dtheta)         (:89-94)
 *   in exactly that expression order.  Fr = I + A: the identity bit for bit except (1,0) and (2,0); Qr = q_pose I; they are
 *   written into the buffer ekf_dense64_propagate_block uploads into.
 *   THEN exactly what ekf_dense64_propagate_block(h, 0, 3, Fr, Qr, dx, ..) launches: the pending rows carried (mapped) or
 *   flushed first as the carry policy says, then its one launch at the live dimension.  The heading is NOT wrapped (:99
 *   does not wrap it).  State, Sigma and the pending rows afterwards are bit for bit those of a twin handle on which
 *   ekf_dense64_propagate_block(h, 0, 3, Fr_out, q_pose I, dx_out, ..) is called.
 *   FAILURES: a NULL handle, then live < 3 -> EKF_ERR_INVALID before the device is looked at, nothing changes.
 *   ONE synchronisation; Fr_out [9] and dx_out [3] (both nullable) come down behind it.  Nothing goes up and no state comes
 *   down.  elapsed_ms (nullable) = HIP-event time of the launches (the operand kernel included).
 * ekf_dense64_measure_landmarks: measurement(sensor_reading, visible_list, .) for landmarks 0 .. n_lm - 1; sensor_xy
 *   [n_lm][2] holds a reading per landmark (read only where visible[i] != 0, and everywhere by a call that initialises).
 *   THE POSE (:109-111) is copied ONCE, at the top of the call, into a 24-byte device slot, and every correction of the call
 *   takes theta, x, y from that slot while the landmark's position comes from the CURRENT state (get_tube_x(i), :152-159).
 *   This is the one difference from the model of ekf_dense64_associate_landmarks, whose reference function re-reads the
 *   pose per reading (:331-333): from the second visible landmark of a call on the two models differ.
 *   *initialised (IN/OUT) is the reference's landmark_init_flag.  0: sensor_xy goes up once and one launch, a thread per
 *   landmark, writes state[3 + 2 i], state[4 + 2 i] for EVERY i < n_lm -- the invisible ones included, as :113-128 do -- from
 *   x + r cos(phi + theta), y + r sin(phi + theta) at the snapshot pose; Sigma is not touched; *initialised becomes 1 once
 *   that launch has completed.  Non-zero: nothing of the sort happens and sensor_xy is read on the host only.
 *   PER VISIBLE LANDMARK, in ascending i: the operands of ekf_dense64_associate_landmarks' correction (cols = {0, 1, 2,
 *   3 + 2 i, 4 + 2 i}, Hc, R = r_meas I, the innovation with its bearing wrapped, :183) at the snapshot pose;
 *   ekf_dense64_correct_sparse, or ekf_dense64_correct_sparse_deferred with EKF_DENSE64_LM_DEFERRED, through their internal
 *   path (the eager one flushes pending rows first, the deferred one only when its two rows do not fit);
 *   state[0] = normalize_angle(state[0]) stored unconditionally (:187); the correction's own synchronisation.
 *   Hc_out [V][2][5] and nu_out [V][2] (nullable; V = the number of visible landmarks) receive the operands of the v-th
 *   correction.  State, Sigma and the pending rows afterwards are bit for bit those of a twin handle on which the host
 *   calls ekf_dense64_correct_sparse[_deferred] with those operands, cols as above and R = r_meas I, and sets the heading.
 *   FAILURES: checked before the device is looked at, in this order: NULL handle; NULL sensor_xy, visible or initialised;
 *   n_lm < 1 or 3 + 2 n_lm > live; a flag bit other than EKF_DENSE64_LM_DEFERRED (EKF_DENSE64_LM_GROW_LIVE included) ->
 *   EKF_ERR_INVALID, nothing changes.  A singular or non-finite S returns EKF_ERR_STATE from that correction: state, Sigma
 *   and the pending rows are as before that correction, the heading is not rewritten, earlier corrections (and the
 *   initialisation) stand, later landmarks are not reached.  *corrected_out (nullable) = corrections completed.
 *   SYNCHRONISATION: one per visible landmark; a call with nothing visible has one.  A reading goes up as sixteen bytes of
 *   kernel arguments; no state comes down.  No floating-point atomics; the same inputs give the same bits on every run.
 *   Memory: the operand buffers of the sparse correction, the scoring buffer of ekf_dense64_score_sparse (32 bytes for the
 *   pose slot and 16 n_lm for the readings of an initialising call), the pending panels with EKF_DENSE64_LM_DEFERRED.
 *   elapsed_ms (nullable) = HIP-event time of the launches, summed over the corrections, a refused one included. */
ekf_status ekf_dense64_predict_landmarks(ekf_dense64_handle h, const ekf_params* params, double dtheta, double dx,
                                         double* Fr_out /* [3][3] nullable */, double* dx_out /* [3] nullable */,
                                         double* elapsed_ms);
ekf_status ekf_dense64_measure_landmarks(ekf_dense64_handle h, const ekf_params* params, int n_lm,
                                         const double* sensor_xy /* [n_lm][2] */, const uint8_t* visible /* [n_lm] */,
                                         int* initialised /* IN/OUT: landmark_init_flag */, unsigned flags,
                                         int* corrected_out /* corrections completed, nullable */,
                                         double* Hc_out /* [V][2][5] nullable */, double* nu_out /* [V][2] wrapped, nullable */,
                                         double* elapsed_ms);

/* Carrying the pending rows across ticks: the caller chooses the flush cadence.  With the policy off (the default) every
 * entry point does exactly what is written above.  With it on and rows pending, the three calls a SLAM tick makes between
 * its corrections no longer flush:
 *   ekf_dense64_propagate_block  runs its one launch on Sigma_base with the same arithmetic and the same bits as on a
 *     handle with nothing pending (Qr goes into Sigma_base alone, the state gets dx as before) and replaces, in every
 *     pending row q < p of BOTH panels, the entries [first, first + r) by Fr times those entries;
 *   ekf_dense64_init_block  runs its one launch on Sigma_base and sets, in every pending row of both panels, the entries
 *     [first, first + r) to G v[cols] (to +0 with s = 0);
 *   ekf_dense64_get_sigma_block  returns Sigma_cur[rows[a]][cols[c]] and stays read-only.
 * This is exact algebra, not an approximation: both updates are Sigma <- A Sigma A^T + Q with A the identity except in the
 * block's r rows, and A Sigma_cur A^T + Q = (A Sigma_base A^T + Q) - sum_q (A K^T[q]) (A T[q]^T)^T.  The extra work is at
 * most 128 rows * r * s multiply-adds in one small launch; there is no pass over Sigma.
 * ekf_dense64_correct_sparse_deferred, ekf_dense64_score_sparse, ekf_dense64_flush and ekf_dense64_pending are unchanged;
 * propagate, correct, score, correct_sparse and get_sigma still flush first; ekf_dense64_set with a Sigma still drops the
 * rows.  With the policy on and nothing pending the three calls launch exactly what they launch with it off.  A refused
 * call (bad arguments, checked before the device is looked at, as above) changes nothing, the pending rows included.
 * ekf_dense64_swap_blocks (below) is carried in the same way: the pending rows take its permutation.
 * ekf_dense64_set_carry never touches Sigma, the state or the pending rows: it only decides what the next calls do, so it
 * may be switched with rows pending.  on: 0 = off, anything else = on.  A NULL handle or NULL pointer returns
 * EKF_ERR_INVALID.
 * ORDER OF ARITHMETIC (part of the contract).  Panel map, for each pending row v of the K panel and of the T panel alike:
 *   v'[first + a] = sum_k M[a][k] v[src[k]]      M = Fr, src = the block (r terms) / M = G, src = cols (s terms)
 * accumulated from +0 in ascending k with one fused multiply-add per term, an order that does not depend on N, ld, first,
 * p or the launch geometry; propagate_block's map is in place, all r source entries of a row being read before any is
 * written.  Readout: x = Sigma_base[i][j]; x = fma(-K^T[q][i], T[q][j], x) for q = 0, 1, .. p - 1 -- the fold of the
 * deferred calls above, so ekf_dense64_get_sigma_block(cols, cols) returns bit for bit the s x s block that
 * ekf_dense64_score_sparse and the next deferred correction work on.  No floating-point atomics: the same bits from run to
 * run.  The padding of the panels (columns >= N) stays zero.  A carried sequence agrees with the flush-first sequence to
 * rounding, not in bits; in particular the corner written by ekf_dense64_init_block (computed from Sigma_base, the pending
 * rows' share of it living in the mapped panels) is bit-equal to the S_out of ekf_dense64_score_sparse taken before the
 * call only when nothing is pending. */
ekf_status ekf_dense64_set_carry(ekf_dense64_handle h, int on);
ekf_status ekf_dense64_get_carry(ekf_dense64_handle h, int* on);

/* The live dimension: the cost of the structured calls follows the map, not the handle's capacity.  A handle is created
 * once at the capacity N it will ever need; with live = Na < N the STRUCTURED calls -- ekf_dense64_propagate_block,
 * ekf_dense64_correct_sparse, ekf_dense64_correct_sparse_deferred, ekf_dense64_score_sparse, ekf_dense64_init_block,
 * ekf_dense64_swap_blocks and ekf_dense64_flush, with the panel map and the read-through of ekf_dense64_set_carry -- treat it as the filter of dimension
 * Na that lives in Sigma[0:Na, 0:Na] and state[0:Na]: every launch of theirs is cut for Na (a flush rewrites 16 Na^2 bytes,
 * not 16 N^2), and
 *   NOTHING OUTSIDE IS READ OR WRITTEN: no entry of Sigma with a row or column index >= Na and no state entry >= Na, neither
 *   the padding nor the entries between Na and the next multiple of 16 / 64 / 128 that the kernels' tiles cover (there the
 *   loads and stores are masked element by element; what the workspace and the pending panels hold at indices >= Na from
 *   wider calls reaches no stored value).
 * The order of arithmetic of every structured call is independent of N and ld (the contracts above), so the results in the
 * live corner -- Sigma, state, S, nis, flags, the pending count -- are BIT FOR BIT those of a handle created with N = Na
 * that holds the same corner.
 * WHY THE POLICY IS EXACT FOR A GROWING MAP.  If the tail is decoupled, Sigma[i][j] = 0 whenever exactly one of i, j is
 * >= Na, the full-width call computes T = H Sigma and K = Sigma H^T S^-1 as zero at every index >= Na (H has no column
 * there), so it changes nothing outside the corner and the live call equals it by value everywhere.  The reference's prior
 * and ekf_dense64_init_block with s = 0 both give exactly such a tail, and landmarks are appended in discovery order, so
 * live = 3 + 2 * known is exact.  This is a property of the caller's Sigma, not a check made at run time:
 * ekf_dense64_coupling is the check.
 * Arguments: with live = Na an index >= Na in cols, or a block with first + r > Na (and m, r or s larger than Na allows),
 * returns EKF_ERR_INVALID in the existing order of checks, before the device is looked at; nothing changes, the pending rows
 * included.  ekf_dense64_get_sigma_block, ekf_dense64_get_state_block and ekf_dense64_set_state_block keep their range
 * [0, N); with the carry policy on and rows pending, an entry with a row or column index >= Na is returned as stored (the
 * pending rows have no support there).
 * Pending rows: growing Na never flushes and is exact -- a pending row is zero on [Na_old, ld) whatever the panels held there
 * before; the call sets those columns of the waiting rows to zero.  Shrinking Na flushes first, at the old width.
 * ekf_dense64_set with a Sigma drops the rows as before and leaves the live setting alone, as it leaves the carry policy.
 * The dense-operand calls -- propagate, correct, score, get_sigma, set -- are defined on all N states and stay full-width:
 * they flush first as they always did (at the live width: that is where the rows have support) and ignore the setting.
 * Default live = N: every entry point launches exactly what it launched before the setting existed.  A NULL handle or
 * pointer, Na < 1 or Na > N return EKF_ERR_INVALID.
 * ekf_dense64_coupling: over the entries Sigma[i][j], i, j < N, with exactly one index >= Na: *nonzero = how many are != 0
 * (-0.0 is zero; a NaN counts), *max_abs (nullable) = the largest absolute value, 0 when there is none, NaN if any entry is
 * a NaN.  The check to run before shrinking (ekf_dense64_swap_blocks below says how a block in mid-map gets to the end of
 * the live corner and out of it), or after building a Sigma by other means.  One streaming launch that reads
 * 16 Na (N - Na) bytes, the rectangle under the diagonal as rows; integer counts and an integer maximum of bit patterns,
 * no floating-point atomics: a run repeats bit for bit.  It needs Sigma in memory, so it flushes first like get_sigma;
 * otherwise read-only.  1 <= Na <= N, Na = N gives 0; it does not look at the live setting.  elapsed_ms (nullable) =
 * HIP-event time of the launches. */
ekf_status ekf_dense64_set_live(ekf_dense64_handle h, int Na);      /* 1 <= Na <= N; default N */
ekf_status ekf_dense64_get_live(ekf_dense64_handle h, int* Na);
ekf_status ekf_dense64_coupling(ekf_dense64_handle h, int Na,
                                long long* nonzero,  /* entries Sigma[i][j] != 0 with exactly one of i, j >= Na */
                                double* max_abs,     /* largest |Sigma[i][j]| among them (0 when none); nullable */
                                double* elapsed_ms);

/* A LOCAL REGION: the live corner made exact for a COUPLED tail (the compressed EKF, Guivant & Nebot 2001).  The live
 * dimension is exact only while the tail is decoupled; on a surveyed map every correction owes the whole of Sigma.  Between
 * ekf_dense64_region_begin(h, Na) and ekf_dense64_region_end the structured calls run at live = Na on A = [0, Na) exactly as
 * they do with ekf_dense64_set_live(Na) -- the corner Sigma_aa, x_a and every returned S, nis and flag are BIT FOR BIT
 * those -- and three accumulators (Phi, Na x Na, from I; Psi, Na x Na, from 0; theta, Na, from 0) record what the rest
 * B = [Na, N) of the map will owe.  With Sigma0 = Sigma as stored at region_begin the region keeps
 *   Sigma_ab = Phi Sigma0_ab    Sigma_ba = Sigma0_ba Phi^T    Sigma_bb = Sigma0_bb - Sigma0_ba Psi Sigma0_ab
 *   x_b = x0_b + Sigma0_ba theta
 * and region_end pays B once: that is exact algebra, not an approximation (for a Sigma_aa that is symmetric; for one that
 * is not symmetric in bits Sigma_ba is taken as Sigma0_ba Phi^T where the eager sequence gives Sigma0_ba Gamma,
 * Gamma = prod (I - H_a^T S^-1 T_a), which differs from Phi^T at rounding level: DESIGN.md 4.8.21).
 * What a call inside a region adds, behind its own launches, on the handle's stream and inside its timed region:
 *   a correction (correct_sparse, correct_sparse_deferred -- at the call, where its gain exists; measure_landmarks and
 *   associate_landmarks without EKF_DENSE64_LM_JOSEPH): with the gain K_a, S^-1 and nu the live call used, and the Phi from
 *   before the call, W = Hc Phi[cols, :], Z = S^-1 W; theta += Z^T nu; Psi += W^T Z; Phi -= K_a W.  32 Na^2 bytes.  A
 *   refused correction (EKF_ERR_STATE) adds nothing.
 *   propagate_block(first, r, Fr) and predict_landmarks: Phi[b, :] <- Fr Phi[b, :], b = [first, first + r); Q and dx do
 *   not reach B.      init_block(first, r, s, cols, G): Phi[b, :] <- G Phi[cols, :], zeros at s = 0.
 *   score_sparse, score_landmarks, flush, get_sigma_block / get_state_block / set_state_block with every index < Na: nothing.
 * Every sum runs in ascending index, one fused multiply-add per term, no floating-point atomics: a run repeats bit for
 * bit, and nothing before region_end depends on N or ld.  Entries between Na and a tile's edge are masked element by
 * element, as the live launches do.
 * EVERY OTHER CALL ENDS THE REGION FIRST and then runs as it always did, so no result is ever stale: get_sigma, get_state,
 * set, set_state, propagate, correct, score, swap_blocks, health, symmetrize, factor, coupling, map_congruence,
 * reframe_landmarks, join_congruence, join_map, extract_map (on either handle), score_landmark_pairs, merge_landmarks, score_readings, joint_operands, associate_joint,
 * associate_scan, associate_scan_joint, correct_sparse_joseph and EKF_DENSE64_LM_JOSEPH, set_live (also the one inside
 * EKF_DENSE64_LM_GROW_LIVE), and a block readout or state block with an index >= Na.  Such a call checks its arguments
 * first, against the live dimension the region found -- a REFUSED call ends nothing, the region stays open -- and the
 * global update then runs on the handle's stream INSIDE that call's own timed region, ahead of its own launches: its
 * elapsed_ms includes it (the calls without a timed region -- get_state, set_state, set, set_live, the block readouts --
 * just run it first).  ekf_dense64_region_info counts these endings.
 * ekf_dense64_region_begin: 3 <= Na < N (EKF_ERR_INVALID otherwise); EKF_ERR_STATE when a region is open.  The pending rows
 * are applied first, at the old width; the live value is remembered and live = Na.  The accumulators (2 Na pitch + 129 pitch
 * doubles, pitch = Na rounded up to 128) and the scratch of the global update (2 Na ld doubles) come from the handle's
 * ledger as ONE all-or-nothing group and stay for the next region that needs no more; on a failure the call returns
 * EKF_ERR_NOMEM (EKF_ERR_HIP for another error), the HIP error is cleared, no region is open and the handle is otherwise as
 * it was.
 * ekf_dense64_region_end: EKF_ERR_STATE when no region is open.  The pending rows are applied at width Na, then, in this order
 * because the first two read Sigma0_ab and Sigma0_ba:  x_b += Sigma0_ba theta;  Y = -(Psi Sigma0_ab) and V = Phi Sigma0_ab
 * into the scratch;  Sigma_bb += Sigma0_ba Y on the fp64 MFMA tile of the dense propagation, on Sigma's own 128-grid with
 * K = Na rounded up to 16 -- 2 Na (N - Na)^2 flop, the one large product; operands outside the product are answered with
 * zeros AT THE LOAD and no entry with a row or column index < Na (or in the padding) is stored, so a NaN or an Inf in
 * Sigma_bb or Sigma_aa reaches nothing it does not belong to;  Sigma_ba <- Sigma0_ba Phi^T through the scratch;
 * Sigma_ab <- V.  The padding of Sigma and of the state stays +0.  The remembered live value is restored.  *report
 * (nullable): what the region was and absorbed.  elapsed_ms (nullable) = HIP-event time of the launches. */
typedef struct {
    int Na, Nb;                  /* the region and the rest, Nb = N - Na */
    long long corrections;       /* corrections absorbed (refused ones not counted) */
    long long row_maps;          /* propagate_block / init_block calls absorbed */
    long long group_bytes;       /* device bytes of the accumulators and the scratch */
} ekf_dense64_region_report;
ekf_status ekf_dense64_region_begin(ekf_dense64_handle h, int Na, double* elapsed_ms);
ekf_status ekf_dense64_region_end(ekf_dense64_handle h, ekf_dense64_region_report* report, double* elapsed_ms);
/* every output nullable; *Na = 0 without a region; corrections and row_maps: of the open region, or of the last one */
ekf_status ekf_dense64_region_info(ekf_dense64_handle h, int* active, int* Na, long long* corrections, long long* row_maps,
                                   long long* ended_by_other_call);
/* Test hook: Sigma as it sits in memory, ld x ld doubles row-major (ld from ekf_dense64_launch_info), and the state, ld
 * doubles, padding included -- every call of the handle keeps the padding at +0, and this is how a test looks at it.
 * Either output nullable.  It needs Sigma in memory: pending rows are applied and an open region ends first. */
ekf_status ekf_dense64_get_padded(ekf_dense64_handle h, double* sigma_out, double* state_out);
/* the plan of a region of Na states on this handle (every output nullable): the tile of the accumulator pass and its
 * workgroup, the row pitch of Phi and Psi, the tiles of that pass, the 128 x 128 tiles and the K of the Sigma_bb product,
 * the bytes of the group */
ekf_status ekf_dense64_region_launch_info(ekf_dense64_handle h, int Na, int* tile_rows, int* tile_cols, int* threads,
                                          int* pitch, int* update_tiles, int* gemm_tiles, int* gemm_k,
                                          long long* group_bytes);

/* (Re)initialisation of a block of states: what a map that grows, or a fixed-capacity map that recycles a slot, does to
 * Sigma.  The states b = [first, first + r) are replaced by a new variable y = g(x[cols], z) of s other states and a
 * reading z: G (r x s) is the Jacobian of g with respect to x[cols], W the caller's Gz R Gz^T, xb the value g(..).  The
 * call gives what ekf_dense64_propagate(h, 1, ..) gives with
 *   F = identity except F[b, b] = 0 and F[b, cols] = G          Q = zero except Q[b, b] = W
 * that is
 *   Sigma[b, j] <- sum_k G[a][k] Sigma[cols[k]][j]   for every column j outside b   (s ROWS of Sigma are read)
 *   Sigma[i, b] <- sum_k Sigma[i][cols[k]] G[a][k]   for every row i outside b      (s COLUMNS: Sigma is never symmetrised)
 *   Sigma[b, b] <- (G Sigma[cols, cols]) G^T + W     (the inner r x s product rounded to fp64 first; W by one plain
 *                                                     addition; W = NULL: no addition)
 *   state[first + k] <- xb[k]                        when xb is given
 * and nothing else is written: the old content of the block's rows and columns is not read and does not leak into the
 * result, the padding of Sigma and of the state stays zero, the F and Q of ekf_dense64_set are neither read nor changed.
 * s = 0 (cols = G = NULL) drops the block: its rows and columns become +0, its corner W, and Sigma is not read at all.
 * With W = 100 I that is the prior the reference's constructor gives every landmark (ekf_slam.cpp:27-36), and with xb from
 * initialize_landmark (:200-214) the whole of the reference's initialisation; s = 3, cols = {0, 1, 2} and G the derivative
 * of the inverse sensor model with respect to the pose is the textbook correlated initialisation (INTEGRATION.md spells
 * both).  32 (r + s) N bytes move instead of ekf_dense64_set's 8 N^2 or a dense propagation with an embedded F.
 * 1 <= r <= min(N, EKF_DENSE64_MAX_R), 0 <= s <= min(N - r, EKF_DENSE64_MAX_S), 0 <= first, first + r <= N; cols: distinct
 * indices in [0, N), none of them inside b.  Lists that overlap b are not supported: the in-place case cols = b is
 * ekf_dense64_propagate_block.  A NULL handle (checked first), a bad first, r or s, NULL cols or G with s > 0, an index
 * that is negative, out of range, repeated or inside b return EKF_ERR_INVALID before the device is looked at; Sigma and the
 * state are then as they were.
 * ORDER OF ARITHMETIC (part of the contract): every entry is a dot product of exactly s terms, accumulated from +0 in
 * ascending k of the list with one fused multiply-add per term; the corner is
 *   S[a][d] = (sum_k T'[a][k] G[d][k]) + W[a][d],   T'[a][k] = sum_j G[a][j] Sigma[cols[j]][cols[k]]  rounded to fp64
 * the order ekf_dense64_score_sparse uses for S: the new corner is bit for bit the S_out of
 * ekf_dense64_score_sparse(h, 1, r, s, cols, G, W, ..) taken before the call.  One launch, no floating-point atomics, an
 * order that does not depend on N, ld, first or the launch geometry: the same source values give the same bits wherever
 * they sit, whatever N is, on every run.
 * Memory: 66 KB of operands (G, W, xb, cols) allocated with the handle; the call allocates nothing.  Model-free (g, its
 * Jacobians and any wrapping of an angle stay with the caller), synchronous, on the handle's stream.  elapsed_ms
 * (nullable) = HIP-event time of the launch only. */
ekf_status ekf_dense64_init_block(ekf_dense64_handle h, int first, int r, int s,
                                  const int* cols,     /* [s] distinct, in [0, N), none inside [first, first + r); NULL iff s == 0 */
                                  const double* G,     /* r x s row-major; NULL iff s == 0 */
                                  const double* W,     /* r x r row-major, NULL = no addition */
                                  const double* xb,    /* r: state[first + k] = xb[k]; NULL = state untouched */
                                  double* elapsed_ms); /* HIP-event time of the launch only (nullable) */

/* Exchange of two blocks of states: what a map that REMOVES a landmark in its middle does to Sigma.  The call is the
 * symmetric permutation Sigma <- P Sigma P^T, state <- P state for the P that swaps A = [first_a, first_a + r) with
 * B = [first_b, first_b + r) and is the identity elsewhere; with k, l in [0, r):
 *   Sigma[first_a + k][j] <-> Sigma[first_b + k][j]   for every column j outside A u B
 *   Sigma[i][first_a + k] <-> Sigma[i][first_b + k]   for every row i outside A u B
 *   new Sigma[A, A] = old Sigma[B, B] and vice versa; new Sigma[first_a + k][first_b + l] = old Sigma[first_b + k][first_a + l]
 *   and vice versa (the off-diagonal blocks are exchanged, NOT transposed: Sigma is never symmetrised)
 *   state[first_a + k] <-> state[first_b + k]
 * and nothing else is read or written.  It is a pure copy: every entry keeps its bits, NaN payloads and -0.0 included; the
 * padding of Sigma and of the state stays zero; the F and Q of ekf_dense64_set are neither read nor changed.  The argument
 * order (a, b) or (b, a) gives the same result, and the call is its own inverse.  64 r N bytes move, instead of the 16 N^2
 * of ekf_dense64_get_sigma and ekf_dense64_set or a dense propagation with a permutation for F.
 * REMOVING LANDMARK i of a map whose live corner ends with block `last` (INTEGRATION.md spells it):
 *   ekf_dense64_swap_blocks(h, first_i, first_last, r, ..)      unless i is the last block itself
 *   ekf_dense64_init_block(h, first_last, r, 0, NULL, NULL, W, NULL, ..)   the block is dropped: decoupled, its corner W
 *   ekf_dense64_set_live(h, Na - r)
 * with the same exchange in the caller's own bookkeeping (its copy of the state, its landmark ids); ekf_dense64_coupling is
 * the check.  Nothing of size N^2 moves except the flush that shrinking already performs.
 * 1 <= r <= EKF_DENSE64_MAX_R; both blocks inside the live dimension, 0 <= first, first + r <= Na; the blocks disjoint,
 * |first_a - first_b| >= r (adjacent blocks are allowed; first_a == first_b is not a swap and is refused).  A NULL handle
 * (checked first) or any bad value returns EKF_ERR_INVALID before the device is looked at; Sigma, the state and the pending
 * rows are then as they were.
 * PENDING ROWS.  With the carry policy off, or nothing pending, the call flushes first, as ekf_dense64_init_block does.  With
 * it on and rows pending nothing is flushed: P is a congruence with A = P, the identity outside the two blocks, so
 * P Sigma_cur P^T = P Sigma_base P^T - sum_q (P K^T[q]) (P T[q]^T)^T -- the launch runs on Sigma_base, and one small launch
 * exchanges the entries [first_a, +r) and [first_b, +r) of every pending row q < p of BOTH panels (a pure copy, all of a
 * row's loads before its stores; the panels' padding and their rows >= p are not touched).  The read-through fold is one
 * fma per pending row per entry and does not depend on position, so after a carried swap ekf_dense64_get_sigma_block and
 * ekf_dense64_score_sparse on index lists permuted by P return bit for bit what they returned on the original lists before
 * it, and the flush gives bit for bit the swap of what it would have given.
 * LIVE DIMENSION.  The launch is cut for live = Na: nothing at an index >= Na is read or written, and the result is the bits
 * of a handle created with N = Na.
 * One launch of 1 + 2 ceil(Na / 64) workgroups (the 2 r x 2 r intersection with the state, the row panel and the column
 * panel in strips of 64); every entry has exactly one partner and one thread owns the pair, so there is no staging, no
 * atomics and no dependence on the launch geometry.  The call allocates nothing and sends nothing up.  Synchronous, on the
 * handle's stream.  elapsed_ms (nullable) = HIP-event time of the launches only. */
ekf_status ekf_dense64_swap_blocks(ekf_dense64_handle h, int first_a, int first_b, int r,
                                   double* elapsed_ms); /* HIP-event time of the launches only (nullable) */

/* Duplicate landmarks: find them, merge them.  The reference's rule creates a landmark whenever the best score of a reading
 * is >= gate_new (ekf_slam.cpp:300-327), so one reading taken at a drifted pose leaves a second copy of an existing tube in
 * the map.  The repair is a landmark-to-landmark Mahalanobis test, a fusion of the two states and the removal of one.
 * State layout as everywhere: landmark i sits at 3 + 2 i, 4 + 2 i.
 * ekf_dense64_score_landmark_pairs: ALL pairs of the first n_lm landmarks in one pass over Sigma's landmark corner
 * (8 (3 + 2 n_lm)^2 bytes read once; ekf_dense64_score_sparse takes 65536 rows a call, all pairs of 5000 landmarks would
 * be about 380 calls).  DEFINITION: for a < b, d2(a, b) is the nis ekf_dense64_score_sparse returns, bit for bit, for
 *   m = 2, s = 4, cols = {3 + 2a, 4 + 2a, 3 + 2b, 4 + 2b}, Hc = [[1, 0, -1, 0], [0, 1, 0, -1]], R = r_merge I,
 *   nu = x[3 + 2a .. 4 + 2a] - x[3 + 2b .. 4 + 2b]   (one plain subtraction each)
 * under that call's ORDER OF ARITHMETIC: fused multiply-adds from +0 in ascending k, so T[0][j] = fl(Sigma[a0][j] -
 * Sigma[b0][j]) and S[0][0] = fl(T[0][a0] - T[0][b0]) + R; Sigma is never symmetrised (the blocks Sigma_ab and Sigma_ba
 * both enter); the elimination and the quadratic form are those of that call at m = 2, with its pivot rule (largest
 * |entry|, lowest row on a tie) and its verdict (non-finite S, zero or non-finite pivot, non-finite inverse: the pair is
 * FLAGGED and its d2 is a NaN).  d2(b, a) = d2(a, b) in bits (every operand is negated exactly).
 *   nearest[a]  the partner b != a with the smallest d2(min(a, b), max(a, b)); the lowest index on equal scores; a flagged
 *               pair never wins; -1 with no valid partner (n_lm = 1, or every pair of a flagged)
 *   d2[a]       that score, +Inf with no valid partner
 *   *n_below    (nullable) unordered pairs with d2 < gate          *n_flagged  (nullable) flagged pairs
 * At least one of nearest, d2 is given.  Integer counters and a pure (min, lowest index) argmin, no floating-point atomics:
 * every order of reduction gives the same bits and a run repeats bit for bit.
 * The call is read-only on Sigma and the state.  It needs Sigma in memory, so it FLUSHES THE PENDING ROWS FIRST, after its
 * own argument checks, as ekf_dense64_coupling does.  1 <= n_lm and 3 + 2 n_lm <= live; nothing at an index >= 3 + 2 n_lm
 * is read (Sigma, state, padding: the tiles' loads are masked element by element), so the results are those of a handle
 * created with N = 3 + 2 n_lm that holds the same corner.  A NULL handle (checked first), nearest and d2 both NULL, a bad
 * n_lm, an r_merge that is negative or not finite, a NaN gate return EKF_ERR_INVALID before the device is looked at and
 * change nothing, the pending rows included.  The workspace (12 bytes per landmark and tile of 32, about 9.5 MB at
 * n_lm = 5000) is allocated by the first call and grows with n_lm; a failure there returns EKF_ERR_NOMEM and leaves the
 * handle as it was.  Two launches (a workgroup per tile (A <= B) of 32 x 32 pairs, then a fold per landmark), one
 * synchronisation; ekf_dense64_pairs_launch_info reports the tile side in landmarks and the workgroup size.
 * elapsed_ms (nullable) = HIP-event time of the launches, the flush included.
 * ekf_dense64_merge_landmarks: landmarks a and b (either order; lo = min, hi = max) become one, a layer over the calls
 * above with no arithmetic of its own: a one-thread kernel writes the operands of the definition for (lo, hi) on the device
 * (no state comes down) -- cols, Hc and R as they stand, and for the innovation that of the reading z = 0 of x_lo - x_hi,
 * z - H x = x_hi - x_lo, the exact negative of the definition's nu, so S and nis keep their bits and the correction pulls
 * the two copies together --, ekf_dense64_correct_sparse -- with EKF_DENSE64_LM_DEFERRED ekf_dense64_correct_sparse_deferred
 * -- applies them (the constraint x_lo = x_hi with noise r_merge I), and hi is removed by the recipe of
 * ekf_dense64_swap_blocks: swap_blocks(hi, last) unless hi is the last known landmark, init_block(last, s = 0,
 * W = sigma0_landmark I), --*known; with EKF_DENSE64_LM_GROW_LIVE also ekf_dense64_set_live(3 + 2 *known).  The same
 * internal paths run, so carry, pending rows and live behave as in that sequence spelled by the caller, and the result is
 * bit for bit the spelled sequence's.  *moved_from (nullable) = the old index of the landmark that now sits in slot hi, -1
 * when hi was the last (the library keeps no ids: the caller's bookkeeping follows it).  *d2_out (nullable) = the
 * correction's nis: the bits of the scan's d2(lo, hi) when nothing changed in between.  A singular S (r_merge = 0 on
 * perfectly correlated copies) returns EKF_ERR_STATE with the state, Sigma, the pending rows and *known untouched.  A NULL
 * handle or known, the known landmarks outside the live dimension, a == b, an index outside [0, *known), a bad r_merge,
 * unknown flag bits return EKF_ERR_INVALID before the device is looked at.  params: NULL = the reference's constants (only
 * sigma0_landmark is used).  elapsed_ms (nullable) = HIP-event time of the launches of every leg. */
ekf_status ekf_dense64_pairs_launch_info(ekf_dense64_handle h, int* tile_landmarks, int* threads);
ekf_status ekf_dense64_score_landmark_pairs(ekf_dense64_handle h, int n_lm, double r_merge, double gate,
                                            int* nearest /* [n_lm], nullable */, double* d2 /* [n_lm], nullable */,
                                            long long* n_below, long long* n_flagged, double* elapsed_ms);
ekf_status ekf_dense64_merge_landmarks(ekf_dense64_handle h, const ekf_params* params, int a, int b, double r_merge,
                                       int* known, int flags /* EKF_DENSE64_LM_DEFERRED | EKF_DENSE64_LM_GROW_LIVE */,
                                       int* moved_from, double* d2_out, double* elapsed_ms);
/* ekf_dense64_remove_landmark: the removal half of ekf_dense64_merge_landmarks as a call of its own -- landmark i of *known
 * is dropped by the recipe of ekf_dense64_swap_blocks: swap_blocks(i, last) unless i is the last known landmark,
 * init_block(last, s = 0, W = sigma0_landmark I), --*known; with EKF_DENSE64_LM_GROW_LIVE (the only flag it knows) also
 * ekf_dense64_set_live(3 + 2 *known).  The same internal function as the merge's: carry, pending rows and live behave as in
 * that sequence spelled by the caller, the result is its result bit for bit, and inside an open region the three calls do
 * what they do when spelled there.  *moved_from (nullable) as in the merge: the old index of the landmark that now sits in
 * slot i, -1 when i was the last.  A NULL handle (first) or known, the known landmarks outside the live dimension, an i
 * outside [0, *known), unknown flag bits return EKF_ERR_INVALID before the device is looked at and change nothing.  params:
 * NULL = the reference's constants (only sigma0_landmark is used).  elapsed_ms (nullable) = HIP-event time of every leg. */
ekf_status ekf_dense64_remove_landmark(ekf_dense64_handle h, const ekf_params* params, int i, int* known /* IN/OUT */,
                                       unsigned flags /* EKF_DENSE64_LM_GROW_LIVE */, int* moved_from, double* elapsed_ms);

/* WHICH landmark is spurious: a laser scan cast against the handle's own map.  A landmark that stands where no tube is (a
 * noise cluster, a tube that was moved, a reading taken at a drifted pose) is never observed again and never goes away; the
 * scan that arrives every tick says so: a beam that returns from BEHIND the place where a mapped tube should stand has seen
 * through it, a beam that returns from its surface supports it, a beam that returns short of it says nothing (something
 * unmapped is in the way).  The beams carry this where the circle pipeline cannot: a cluster needs more than 6 points, which
 * at 360 beams a tube of radius 0.0762 m gives only within about 1.25 m, and the lidar reaches 3.5 m.
 * ekf_dense64_scan_evidence, for the landmarks [first_lm, first_lm + count) and lidar->n_beams beams:
 * GEOMETRY (model 0 of ekf_lidar_params on the state; the definitions and the order of operations of ekf_simulate_scans
 *   with range_std = 0): beam b leaves (x, y) = state[1..2] in direction th = state[0] + 2 pi b / n_beams (not wrapped),
 *   d = (cos th, sin th); half = border_width / 2 (INFINITY: no wall);  wall_x = (half - x) / d_x for d_x > 0,
 *   (-half - x) / d_x for d_x < 0, +Inf otherwise, wall_y likewise;  r = fmin(fmin(wall_x, wall_y), range_max);  then for the
 *   landmarks j in ascending index  f = (x, y) - m_j,  bq = f_x d_x + f_y d_y,  cq = f_x f_x + f_y f_y - tube_radius^2,
 *   disc = bq bq - cq,  and where disc > 0 the root t = -bq - sqrt(disc) replaces r when 0 < t < r.  Products and sums are
 *   rounded separately.  expected_out[b] = r;  hit_out[b] = the landmark whose root stands, -1 for the wall or range_max.  The
 *   comparison is strict: of equal roots the LOWEST INDEX wins (two landmarks with identical coordinates give every beam to
 *   the lower one), a NaN root never wins, a pose inside a tube has no positive nearest root and so no hit.
 * TOLERANCE  tol_out[i] = tol_abs + kappa sqrt(max(S00_i, 0)), S00_i the range variance of landmark first_lm + i under the
 *   current Sigma, pending rows included: the [0][0] entry of the S ekf_dense64_score_landmarks returns for it, bit for bit
 *   (that call's launches run; R = params->r_meas I, NULL: the reference's constants).  A landmark whose score flag is 1 gets
 *   +Inf: all its beams agree and none count against it.  kappa == 0: tol_abs, the scoring kernel is not launched and Sigma
 *   is not read.  kappa is what keeps a miss on a poorly localised landmark from counting as a miss.
 * CLASSES    class_out[b], with obs = ranges[b], exp = expected_out[b], tol = tol_out[hit_out[b] - first_lm], every
 *   comparison on rounded doubles as written:
 *     4  invalid: obs is a NaN or <= 0 (whatever the beam expects)
 *     0  exp is the wall or range_max; such a beam with obs < exp - tol_abs counts in report->n_unexplained
 *     1  agree: |obs - exp| <= tol        2  through: obs - exp > tol        3  short: exp - obs > tol
 *   n_expected, n_agree, n_through, n_short [count]: per landmark its beams of classes {1, 2, 3}, 1, 2, 3; invalid beams
 *   count in none.  ranges == NULL: the expected scan only, every class and every counter 0.  report: n_candidates = the
 *   landmarks with |f|^2 <= (range_max + tube_radius)^2 (1 + 1e-12) (the only ones a beam can reach; the rest are not walked),
 *   n_on_tube = beams with hit_out >= 0 (invalid ones included, counted without ranges too), n_unexplained, n_invalid.
 * Counters are integers, there are no floating-point atomics and no floating-point sum: a landmark's four counters, its tol
 * and every beam's outputs are the same bits on every run, for any capacity N >= live, for any slice [first_lm, first_lm +
 * count) that holds the landmarks in reach of the beams concerned, and whatever out-of-reach landmarks the map also holds.
 * The call is READ-ONLY and opt-in: the state, Sigma, the pending rows and the factor snapshot keep their bits; NOTHING IS
 * FLUSHED (the deferred path corrects the state at once, the scoring kernel reads through the pending rows); no other
 * entry point launches anything different because it exists.  Inside an open region it behaves as
 * ekf_dense64_rank_landmarks: the region ends first, behind the checks.  It runs on the live corner.  CHECKS, in this order,
 * each EKF_ERR_INVALID before the device is looked at, nothing changed: 1. a NULL handle or lidar; 2. every output NULL;
 * 3. count < 1 or first_lm < 0; 4. 3 + 2 (first_lm + count) > live; 5. n_beams outside [1, EKF_DENSE64_SCAN_MAX_BEAMS];
 * 6. tube_radius or range_max not finite or not > 0; 7. tol_abs or kappa negative or a NaN; 8. model != 0.
 * The ranges go up through the pinned ring of ekf_dense64_fit_scan; the workspace (44 bytes per landmark and 21 KB) is
 * reserved by the first call from the handle's ledger and grows with count; a failure there returns EKF_ERR_NOMEM and
 * leaves the handle as it was.  Launches: per 32768 landmarks (kappa > 0 only) the terms, the scoring kernel and the
 * tolerances, else the tolerances alone; the compaction of the landmarks in reach (one workgroup); a workgroup per
 * beam_tile beams that walks them through LDS lm_chunk at a time (ekf_dense64_evidence_launch_info).  ONE synchronisation,
 * every output comes down behind it.  elapsed_ms (nullable) = HIP-event time of the launches.
 * ekf_dense64_evidence_update: the bookkeeping, no handle and no device.  logodds [count] is the caller's (the library
 * keeps no landmark ids: the array follows *moved_from on merge and remove).  Per landmark with n_expected >= min_beams:
 * a HIT when 2 n_agree >= n_expected: l = l + w_hit, verdict +1; a MISS when 2 n_through > n_expected: l = l - w_miss,
 * verdict -1; otherwise verdict 0; then every l is clamped to [l_min, l_max].  Integer decisions, plain fp64 sums in
 * index order.  verdict_out nullable.  NULL arrays, count < 1, min_beams < 1, a negative or NaN weight, l_min > l_max or a
 * NaN bound return EKF_ERR_INVALID. */
typedef struct ekf_dense64_evidence_report {
    int n_candidates;    /* landmarks within reach of the pose                       */
    int n_on_tube;       /* beams whose expected first hit is a landmark             */
    int n_unexplained;   /* beams expected on wall / range_max that came back short  */
    int n_invalid;       /* observed ranges that are NaN or <= 0                     */
} ekf_dense64_evidence_report;
ekf_status ekf_dense64_evidence_launch_info(ekf_dense64_handle h, int* beam_tile, int* lm_chunk, int* threads);
ekf_status ekf_dense64_scan_evidence(ekf_dense64_handle h, const ekf_params* params, const ekf_lidar_params* lidar,
                                     const double* ranges /* [n_beams], nullable */, int first_lm, int count,
                                     double tol_abs, double kappa, int* n_expected, int* n_agree, int* n_through,
                                     int* n_short /* [count] each, nullable */, double* tol_out /* [count] */,
                                     double* expected_out /* [n_beams] */, int* hit_out /* [n_beams] */,
                                     unsigned char* class_out /* [n_beams] */, ekf_dense64_evidence_report* report,
                                     double* elapsed_ms);
ekf_status ekf_dense64_evidence_update(int count, const int* n_expected, const int* n_agree, const int* n_through,
                                       int min_beams, double w_hit, double w_miss, double l_min, double l_max,
                                       double* logodds /* IN/OUT [count] */, int* verdict_out /* [count], nullable */);

/* Is Sigma still a covariance, and the exact repair of its symmetry.  Every call above keeps the contract "Sigma is never
 * symmetrised" (T = H Sigma is taken from rows, U = Sigma H^T from columns), so rounding lets Sigma[i][j] and Sigma[j][i]
 * drift apart over a long run.  ekf_dense64_health measures that, and what else stops a matrix from being a covariance,
 * without Sigma leaving the device; ekf_dense64_symmetrize makes the two halves equal again, at the caller's own cadence.
 * Both are opt-in: no other entry point calls them or launches anything different because they exist.
 * Both are structured calls: they run on the live corner Sigma[0:Na, 0:Na], Na = live (N by default), and nothing at a row
 * or column index >= Na is read or written (the tiles' loads and stores are masked element by element).  Both need Sigma
 * in memory, so they FLUSH THE PENDING ROWS FIRST, after their own argument checks, as ekf_dense64_coupling does.  Neither
 * touches the state vector.  A bad argument returns EKF_ERR_INVALID before the device is looked at and changes nothing, the
 * pending rows included.
 * ekf_dense64_health: read-only on Sigma, one pass over the corner (8 Na^2 bytes).  DEFINITIONS, all over i, j < Na, every
 * operation in IEEE binary64, round to nearest even, each rounded on its own (fl), subnormals kept:
 *   n_nonfinite   entries Sigma[i][j] that are a NaN or +-Inf (the diagonal included)
 *   n_asym        pairs i < j whose two entries differ in BITS (so -0.0 against +0.0 counts, and two NaNs of different
 *                 payload; two NaNs of the same bits do not)
 *   max_asym, asym_i, asym_j
 *                 with d = fl(Sigma[i][j] - Sigma[j][i]), one plain subtraction per pair i < j: the maximum of |d| taken on
 *                 the 64-bit pattern of |d| (sign bit cleared, compared as an unsigned integer: the order of the values for
 *                 everything that is not a NaN, every NaN above +Inf, NaNs among themselves by payload); max_asym is the
 *                 double of that pattern, so it is a NaN if any d is.  (asym_i, asym_j) is the lexicographically lowest
 *                 (i, j), i < j, that attains the maximum.  With no pair (Na = 1): 0.0 and -1, -1.  A symmetric corner with
 *                 Na >= 2 gives 0.0 at (0, 1).
 *   min_diag, min_diag_i
 *                 the smallest Sigma[i][i] by value among the diagonal entries that are not a NaN; on equal values (-0.0
 *                 equals +0.0) the lowest index wins and min_diag has that entry's bits.  All NaN: +Inf and -1.
 *   n_diag_bad    diagonal entries that are a NaN or <= 0 (-0.0 and +0.0 are <= 0)
 *   n_minor       pairs i < j with fl(Sigma[i][j] * Sigma[j][i]) > fl(Sigma[i][i] * Sigma[j][j]): a negative 2 x 2 principal
 *                 minor, a necessary condition of positive semi-definiteness that costs no further traffic.  Each product
 *                 is rounded once (no fused operation); a comparison that involves a NaN is false and is not counted.
 * A NULL handle (checked first) or a NULL report returns EKF_ERR_INVALID.
 * ekf_dense64_symmetrize: for every pair i < j < Na whose two entries differ in bits, both are set to
 *   v = fl(0.5 * fl(Sigma[i][j] + Sigma[j][i]))      one addition, one halving
 * (the halving is exact unless v is subnormal; a sum that overflows gives +-Inf; a NaN operand gives a NaN with that
 * operand's payload as the hardware's addition hands it on).  A pair whose entries hold the same bits is NOT WRITTEN, so NaN
 * payloads of equal pairs survive; the diagonal is never written.  Afterwards Sigma[i][j] and Sigma[j][i] hold the same bits
 * for all i, j < Na; a second call writes nothing and returns *n_changed = 0; a symmetric corner is only read.
 *   *n_changed (nullable)  the pairs written = n_asym of a health call made just before
 *   *max_asym  (nullable)  as defined above, on the values before the call
 * 8 Na^2 bytes are read and at most 8 Na^2 written, in place: one workgroup owns both tiles of a tile pair, so there is no
 * staging buffer of size Na^2.  A NULL handle returns EKF_ERR_INVALID.
 * Both calls: a workgroup per tile pair (A <= B) of the corner; Sigma[A rows, B cols] is read (and written) along rows,
 * Sigma[B rows, A cols] along rows too, through a transpose in LDS -- no walk down a column of Sigma on either side.
 * Integer counters, an integer maximum of bit patterns, locations that are pure functions of the data (per-tile records and
 * a fold): no floating-point atomics, a run repeats bit for bit.  The workspace (16 bytes per tile pair and 8 per state,
 * about 0.3 MB at Na = 10003) is allocated by the first call and grows with Na; a failure there returns EKF_ERR_NOMEM and
 * leaves the handle as it was.  ekf_dense64_health_launch_info reports the tile side in states and the workgroup size.
 * Synchronous, on the handle's stream.  elapsed_ms (nullable) = HIP-event time of the launches, the flush included. */
typedef struct ekf_dense64_health_report {
    long long n_nonfinite;
    long long n_asym;
    long long n_diag_bad;
    long long n_minor;
    double max_asym;
    double min_diag;
    int asym_i, asym_j;
    int min_diag_i;
    int reserved;   /* 0 */
} ekf_dense64_health_report;
ekf_status ekf_dense64_health_launch_info(ekf_dense64_handle h, int* tile, int* threads);
ekf_status ekf_dense64_health(ekf_dense64_handle h, ekf_dense64_health_report* out, double* elapsed_ms);
ekf_status ekf_dense64_symmetrize(ekf_dense64_handle h, long long* n_changed, double* max_asym, double* elapsed_ms);

/* Which landmark is worth looking at next, and what would that buy?  Every call above reacts to a reading that has
 * arrived; these two answer before it has: for each of `count` landmarks from first_lm on, what ONE hypothetical
 * observation of it with the m = 2 Jacobian H (non-zero in the five columns cols = {0, 1, 2, 3 + 2 i, 4 + 2 i}: H[:, cols[k]]
 * = Hc[:, k]) and the noise R would take off the trace of Sigma, off the three pose variances and off the entropy of the
 * state.  With U = Sigma H^T (Na x 2) and S = H Sigma H^T + R:
 *   drop of tr Sigma                 tr(S^-1 U^T U)
 *   drop of Sigma[0][0] + [1][1] + [2][2]   tr(S^-1 U_p^T U_p), U_p the first three rows of U
 *   drop of the entropy              0.5 (log det S - log det R)
 * Row r of U for landmark i needs Sigma[r][0 .. 2] and Sigma[r][3 + 2 i .. 4 + 2 i] only, so all landmarks together read
 * every element of the live corner ONCE, along rows: 8 Na^2 bytes, the traffic of ekf_dense64_health, instead of one clone
 * and one correction per landmark.  Read-only and opt-in: no other entry point launches anything different because they
 * exist.  Structured calls: they run on the live corner Sigma[0:Na, 0:Na], Na = live, and nothing at a row or column index
 * >= Na is read.  Both need Sigma in memory, so they FLUSH THE PENDING ROWS FIRST, after their own argument checks, exactly
 * as ekf_dense64_health does, and inside an open region they behave as that call does: the region ends first, and
 * ekf_dense64_rank_landmarks builds its Jacobians and ranges from the state the region's end leaves.  Sigma after the flush,
 * the state and the factor snapshot are untouched.
 * DEFINITIONS, for landmark i = first_lm + j, every operation in IEEE binary64, round to nearest even, each rounded on its
 * own (fl; no fused operation except where S says so), with x (+) y = fl(x + y):
 *   u_a[r]  = ((((+0 (+) fl(Sigma[r][cols[0]] Hc[a][0])) (+) fl(Sigma[r][cols[1]] Hc[a][1])) (+) ..) (+) fl(Sigma[r][cols[4]]
 *             Hc[a][4])), a = 0, 1, r < Na: row r of U, taken from ROW r of Sigma (Sigma is never symmetrised)
 *   G00, G01, G11 = sum over r < Na of fl(u_0 u_0), fl(u_0 u_1), fl(u_1 u_1).  THE ORDER OF THE SUM is a function of Na and
 *             tile_rows (ekf_dense64_value_launch_info) alone: from +0 in ascending r inside each block of tile_rows rows
 *             [k tile_rows, (k + 1) tile_rows), then the blocks' sums from +0 in ascending k.  So a landmark's figures are the
 *             same bits for any first_lm / count it is batched in, for any capacity N >= Na of the handle, on every run.
 *   P00, P01, P11 = the same over r = 0, 1, 2 (from +0, ascending)
 *   S, flag = S_out and flag_out of ekf_dense64_score_sparse(J = count, m = 2, s = 5, cols, Hc, R, r_shared = 1) bit for
 *             bit -- the same kernel is launched -- and S^-1 = A is that call's Gauss-Jordan inverse of S
 *   dtrace      = ((fl(A00 G00) (+) fl(A01 G01)) (+) fl(A10 G01)) (+) fl(A11 G11)
 *   dtrace_pose = the same on P
 *   detS        = fl(fl(S00 S11) - fl(S01 S10)).  No logarithm is taken on the device: the entropy drop is
 *             0.5 log(detS / det R), the caller's to form.
 * A landmark with flag 1 (S not finite, singular, or its inverse not finite) has dtrace = dtrace_pose = detS = NaN; S_out
 * holds S as summed.
 * WHAT dtrace MEANS: it is the trace drop of the update on U = Sigma H^T alone.  It equals tr Sigma - tr Sigma+ of
 * ekf_dense64_correct_sparse (nu = 0) up to rounding when the two halves of Sigma hold the same bits, e.g. after
 * ekf_dense64_symmetrize; that call forms Sigma+ = Sigma - U S^-1 T with T = H Sigma from rows, so otherwise the two differ by
 * a term bounded through max_asym of ekf_dense64_health.
 * *best (nullable): the winners among the landmarks with flag = 0 and in_view = 1 -- i_trace, i_pose, i_det are the indices
 * j in [0, count) of the largest dtrace, dtrace_pose and detS, v_* their values; the lowest index wins a tie, a NaN never
 * wins; with nothing eligible the index is -1 and the value a NaN.
 * ekf_dense64_value_operands: model-free, the kernels' own entry point.  Hc [count][2][5] and R [2][2] (shared) are the
 * caller's; in_view [count] (nullable = all 1) only gates the winners.
 * ekf_dense64_rank_landmarks: the reference's model on the handle's own state [theta, x, y, m1x, m1y, ..]: Hc is Hj of
 * measurement() (ekf_slam.cpp:158-166), which depends on pose and landmark alone, bit for bit the Hc_out of
 * ekf_dense64_score_landmarks for any reading; R = params->r_meas I (NULL: the reference's constants); in_view =
 * (predicted range sqrt(dx^2 + dy^2) <= range_max), or 1 for every landmark when range_max <= 0 or a NaN.  in_view_out
 * [count] and Hc_out [count][2][5] (nullable) return what was used.
 * The outputs dtrace, dtrace_pose, detS [count], S_out [count][2][2], flag_out [count] and best are nullable, not all of them
 * (rank_landmarks: in_view_out and Hc_out count as outputs).
 * ARGUMENT CHECKS, before the device is looked at, in this order: a NULL handle; every output NULL; count < 1 or
 * first_lm < 0; 3 + 2 (first_lm + count) > live; a NULL Hc or R (value_operands).  Each returns EKF_ERR_INVALID and changes
 * nothing, the pending rows included.
 * Four launches behind the operands: the sparse scoring, the pass (a workgroup per tile of tile_rows rows x tile_lm
 * landmarks, lane = landmark, 16-byte loads along the rows, one record of six doubles per row tile and landmark), the fold
 * per landmark, the winners.  No floating-point atomics: a run repeats bit for bit.  The workspace (48 count ceil(Na /
 * tile_rows) bytes of records and about 170 bytes per landmark, 19 MB for 5000 landmarks at Na = 10003) is allocated by the
 * first call and grows with use; a failure there returns EKF_ERR_NOMEM and leaves the handle as it was.
 * Synchronous, on the handle's stream.  elapsed_ms (nullable) = HIP-event time of the launches, the flush included. */
typedef struct ekf_dense64_value_best {
    int i_trace, i_pose, i_det;
    int reserved;   /* 0 */
    double v_trace, v_pose, v_det;
} ekf_dense64_value_best;
ekf_status ekf_dense64_value_launch_info(ekf_dense64_handle h, int* tile_rows, int* tile_lm, int* threads);
ekf_status ekf_dense64_value_operands(ekf_dense64_handle h, int first_lm, int count,
                                      const double* Hc /* [count][2][5] */, const double* R /* [2][2] */,
                                      const unsigned char* in_view /* [count], nullable = all */,
                                      double* dtrace, double* dtrace_pose, double* detS, double* S_out /* [count][2][2] */,
                                      int* flag_out, ekf_dense64_value_best* best, double* elapsed_ms);
ekf_status ekf_dense64_rank_landmarks(ekf_dense64_handle h, const ekf_params* params, int first_lm, int count,
                                      double range_max, double* dtrace, double* dtrace_pose, double* detS,
                                      double* S_out /* [count][2][2] */, int* flag_out, ekf_dense64_value_best* best,
                                      unsigned char* in_view_out /* [count] */, double* Hc_out /* [count][2][5] */,
                                      double* elapsed_ms);

/* The Cholesky factor of Sigma on the device: is Sigma positive definite (the sufficient test that n_minor above is not),
 * log det Sigma (the entropy of the map; its change across a correction is the information gain), and through the forward
 * substitution of ekf_dense64_whiten the Mahalanobis distance e^T Sigma^-1 e of the WHOLE map (its NEES against ground
 * truth, Na degrees of freedom).  Opt-in: no other entry point calls these or launches anything different because they
 * exist.
 * ekf_dense64_factor is a structured call on the live corner Sigma[0:Na, 0:Na], Na = live.  THE LOWER TRIANGLE ONLY IS READ:
 * Sigma[i][j] with j <= i < Na, along rows (masked element by element); nothing above the diagonal and nothing at an index
 * >= Na.  The matrix factored is the symmetric matrix with that lower triangle; a caller who wants both halves to count
 * calls ekf_dense64_symmetrize first.  Read-only on Sigma and on the state; it FLUSHES THE PENDING ROWS FIRST, after its
 * argument checks, inside the timed region, as ekf_dense64_health does.  A NULL handle (checked first) or a NULL report
 * returns EKF_ERR_INVALID and changes nothing, the pending rows included.
 * DEFINITION, IEEE binary64, columns j ascending:
 *   d_j     = Sigma[j][j] - sum_{k<j} L[j][k]^2             the pivot
 *   L[j][j] = sqrt(d_j)
 *   L[i][j] = (Sigma[i][j] - sum_{k<j} L[i][k] L[j][k]) / L[j][j]        i > j
 * The square root and the division are the correctly rounded ones, and every quotient is a division by L[j][j] in a forward
 * substitution: there is no inverse of a diagonal block and no multiplication by a reciprocal, so the componentwise bound
 * |Sigma - L L^T|_ij <= gamma_{Na+1} (|L| |L|^T)_ij, gamma_n = n u / (1 - n u), u = 2^-53, holds.  The association of each
 * sum is the implementation's (block columns of 64 states, chains of fused multiply-adds on the matrix cores inside a
 * block update) and depends on (Na, block side) alone; no atomics: a run repeats bit for bit.
 * THE STOP RULE: the first column j whose d_j is not (finite and > 0) ends the factorisation: ok = 0, fail_index = j,
 * fail_pivot = d_j (its bits: +0.0 and -0.0 fail, a NaN keeps its payload), logdet = NaN, min_pivot / max_pivot cover the
 * columns before j.  The call still returns EKF_OK: an indefinite Sigma is a finding, not an error.  The verdict is a pure
 * function of the data -- the lowest failing column -- and a device word that every later launch reads before its first
 * store, so nothing is computed from NaNs.
 * logdet is summed ON THE HOST from the diagonal of L, which comes down with the report: 2.0 * (((log l_0) + log l_1) + ...),
 * ascending, plain binary64 with the C library's log.
 * THE FACTOR IS A SNAPSHOT in a buffer of its own, allocated by the first call and growing with Na: 8 (Na + 63)(Na + 127)
 * bytes at most (Na rounded up to the block side, one block column of workspace beside it), 812.8 MB at Na = 10003.  A
 * failure to allocate returns EKF_ERR_NOMEM and leaves the handle and any earlier snapshot as they were.  Later calls that
 * change Sigma (or the live dimension) neither touch nor invalidate the snapshot: ekf_dense64_get_factor and
 * ekf_dense64_whiten use it as taken.  Before the first factor, and after a factor that ended with ok == 0, both return
 * EKF_ERR_STATE.
 * ekf_dense64_get_factor: L as Na x Na row-major, Na = the dimension the factor was taken at; the strict upper triangle is
 * exactly +0.0.
 * ekf_dense64_whiten: Y[r] = L^-1 B[r] by forward substitution (ascending, divisions by L[j][j]) for 1 <= nrhs <=
 * EKF_DENSE64_WHITEN_MAX_RHS right-hand sides at once, d2[r] = sum_i Y[r][i]^2 (a fixed fold).  A right-hand side gives the
 * same bits alone and at any position of a batch.  With B[r] = state - truth (the caller wraps the heading), d2 is the NEES
 * of the whole map.  EKF_ERR_INVALID before the device is looked at: a NULL handle or B, nrhs out of range, Y_out and d2_out
 * both NULL.  EKF_ERR_STATE: no complete factor, or the snapshot's Na differs from the live dimension.  Read-only on
 * everything but its own operand buffers; it does not read Sigma, so it does NOT flush the pending rows.
 * ekf_dense64_factor_launch_info reports the block side in states (a divisor of 128, >= 16) and the workgroup size.
 * Synchronous, on the handle's stream.  elapsed_ms (nullable) = HIP-event time of the launches, for the factor the flush
 * included. */
typedef struct ekf_dense64_factor_report {
    int    ok;            /* 1: every pivot was finite and > 0, the factor is complete; 0: stopped at fail_index */
    int    fail_index;    /* -1, or the first column j whose pivot was not (finite and > 0) */
    int    min_pivot_i;   /* index of the smallest pivot among the columns factored (lowest index on ties); -1 if none */
    int    Na;            /* the live dimension the factor was taken at */
    double fail_pivot;    /* that pivot's value (bits), 0.0 when ok */
    double min_pivot;     /* smallest / largest d_j = L[j][j]^2 as computed BEFORE the square root, over the */
    double max_pivot;     /*   columns factored; +Inf / 0.0 if none */
    double logdet;        /* ok: 2 * sum_j log(L[j][j]); else NaN */
} ekf_dense64_factor_report;
ekf_status ekf_dense64_factor_launch_info(ekf_dense64_handle h, int* block, int* threads);
ekf_status ekf_dense64_factor(ekf_dense64_handle h, ekf_dense64_factor_report* out, double* elapsed_ms);
ekf_status ekf_dense64_get_factor(ekf_dense64_handle h, double* L_out /* Na x Na row-major */);
#define EKF_DENSE64_WHITEN_MAX_RHS 64
ekf_status ekf_dense64_whiten(ekf_dense64_handle h, int nrhs, const double* B /* [nrhs][Na] */,
                              double* Y_out /* [nrhs][Na], nullable */, double* d2_out /* [nrhs], nullable */,
                              double* elapsed_ms);

/* The other two things a Cholesky factor is for, against the same snapshot: the full solve X = Sigma^-1 B (the information
 * form of the map, the weights of a full-state fusion, conditional means, the gradient of the whole-map NEES) and the
 * colouring product that turns unit normal draws Z into maps drawn from N(state, Sigma).  Opt-in and read-only on the
 * snapshot: no other entry point calls these or launches anything different because they exist.
 * ekf_dense64_solve: X[r] = L^-T (L^-1 B[r]) for 1 <= nrhs <= EKF_DENSE64_WHITEN_MAX_RHS right-hand sides at once.
 * THE FORWARD HALF IS ekf_dense64_whiten's launches as they stand: Y_out and d2_out are bit for bit what ekf_dense64_whiten
 * returns for the same B.  The backward half, IEEE binary64, i descending from Na - 1:
 *   x_i = (y_i - sum_{k>i} L[k][i] x_k) / L[i][i]
 * Every quotient is a correctly rounded division by L[i][i]: no reciprocal and no inverse of a diagonal block, so the
 * componentwise bounds |L^T x - y|_i <= gamma_Na (|L^T| |x|)_i and |Sigma x - b|_i <= gamma_{3 Na + 1} (|L| |L^T| |x|)_i hold.
 * The association of each sum is the implementation's (block columns of 64 states, descending) and depends on (Na, block
 * side) alone; no atomics: a run repeats bit for bit, and a right-hand side gives the same bits alone and at any position
 * of a batch.  With X_out NULL the backward half is not run.
 * ekf_dense64_color: X[r][i] = sum_{k<=i} L[i][k] Z[r][k], and with add_state != 0 X[r][i] = fl(that sum + state[i]), the
 * addition coming last.  Nothing above the diagonal of the snapshot is taken as L.  The sums run in ascending k in a fixed
 * association (fused multiply-adds on the matrix cores left of the diagonal block, plain multiply-adds inside it), no
 * atomics, the same bits at any position of a batch: |x - L z|_i <= gamma_Na (|L| |z|)_i.
 * THE FACTOR IS A SNAPSHOT, THE STATE IS THE CURRENT ONE (state[0 .. Na), read the way ekf_dense64_get_state_block reads it,
 * pending rows or not): keeping the two in step is the caller's business -- call ekf_dense64_factor after the last
 * correction.  THE HEADING OF A SAMPLE (X[r][0]) IS NOT WRAPPED.
 * Both: EKF_ERR_INVALID before the device is looked at, in this order: a NULL handle, a NULL B / Z, nrhs out of range,
 * X_out, Y_out and d2_out all NULL (solve) or a NULL X_out (color).  EKF_ERR_STATE where ekf_dense64_whiten returns it: no
 * complete factor, or the snapshot's Na differs from the live dimension.
 * Neither reads Sigma, neither flushes the pending rows, neither ends an open region; a refusal changes nothing.
 * Synchronous, on the handle's stream; elapsed_ms (nullable) = HIP-event time of the launches.
 * ekf_dense64_solve_launch_info reports the block side in states and the workgroup sizes of the two kernels. */
ekf_status ekf_dense64_solve(ekf_dense64_handle h, int nrhs, const double* B /* [nrhs][Na] */,
                             double* X_out /* [nrhs][Na], nullable */, double* Y_out /* [nrhs][Na], nullable */,
                             double* d2_out /* [nrhs], nullable */, double* elapsed_ms);
ekf_status ekf_dense64_color(ekf_dense64_handle h, int nrhs, const double* Z /* [nrhs][Na] */, int add_state,
                             double* X_out /* [nrhs][Na] */, double* elapsed_ms);
ekf_status ekf_dense64_solve_launch_info(ekf_dense64_handle h, int* block, int* threads_back, int* threads_color);

/* The map in another frame.  A SLAM map is defined up to the frame it was started in; these calls change that frame on the
 * device: Sigma <- J Sigma J^T in place, one streaming pass over the live corner (16 Na^2 bytes, what a correction moves),
 * instead of ekf_dense64_get_sigma, a host product and ekf_dense64_set.  Opt-in: no other entry point calls these or
 * launches anything different because they exist.
 * The Jacobian of a frame change on (theta, x, y, l1x, l1y, ...) is J = D + [C | 0]: D = blockdiag(1, G, G, ..., G) with the
 * 2 x 2 block G (row-major G[4]) on the robot position and on every landmark, and C, Na x 3 row-major, on the pose columns.
 * THE PAIRS ARE (1, 2), (3, 4), ...: ODD-ALIGNED, INDEX 0 STANDS ALONE.
 * ekf_dense64_map_congruence is a structured call on the live corner Sigma[0:Na, 0:Na], Na = live.  NA MUST BE ODD AND >= 3
 * (Na = 3 + 2 n), otherwise EKF_ERR_INVALID.  Nothing at a row or column index >= Na is read or written (loads and stores
 * are masked element by element).  It needs Sigma in memory, so it FLUSHES THE PENDING ROWS FIRST, carry or not, after its
 * argument checks and inside the timed region, as ekf_dense64_health does.  IT DOES NOT TOUCH THE STATE VECTOR.  A NULL
 * handle (checked first), a NULL G or a bad live dimension returns EKF_ERR_INVALID and changes nothing, the pending rows
 * included.  C is nullable.
 * DEFINITION, every operation in IEEE binary64, round to nearest even, each rounded on its own (fl) unless it is written as
 * a fused multiply-add fma(a, b, c) = fl(a b + c); Sigma below is the corner ON ENTRY (after the flush):
 *   1. P = D Sigma D^T, per 2 x 2 block B = Sigma[i..i+1][j..j+1] of two pairs:
 *        Y = G B     Y[r][c] = fma(G[r][1], B[1][c], fl(G[r][0] * B[0][c]))
 *        Z = Y G^T   Z[r][c] = fma(Y[r][1], G[c][1], fl(Y[r][0] * G[c][0]))          P[i+r][j+c] = Z[r][c]
 *      Row 0 and column 0 get the one-sided product: P[0][j+c] = fma(Sigma[0][j+1], G[c][1], fl(Sigma[0][j] * G[c][0])),
 *      P[i+r][0] = fma(G[r][1], Sigma[i+1][0], fl(G[r][0] * Sigma[i][0])), P[0][0] = Sigma[0][0].
 *   2. With Sigma_p the OLD pose rows (3 x Na), Sigma_c the OLD pose columns (Na x 3), Sigma_pp the old 3 x 3 corner:
 *        A  = Sigma_p D^T + Sigma_pp C^T (3 x Na): the first term as the one-sided product of step 1 (column 0: Sigma[k][0]),
 *             then a = fma(Sigma_pp[k][l], C[j][l], a) for l = 0, 1, 2 in ascending order
 *        Bc = D Sigma_c (Na x 3): the one-sided product from the left (row 0: Sigma[0][k])
 *   3. Sigma'[i][j] = P[i][j] + sum_{k<3} C[i][k] A[k][j] + sum_{k<3} Bc[i][k] C[j][k]: six fused multiply-adds into an
 *      accumulator that starts at P[i][j], the C A terms first, k ascending:
 *        acc = fma(C[i][k], A[k][j], acc), k = 0, 1, 2;  acc = fma(Bc[i][k], C[j][k], acc), k = 0, 1, 2
 *   4. C = NULL: the rank-6 part (steps 2 and 3) is SKIPPED, not multiplied by zeros, so Sigma' = P and NaN payloads in P
 *      survive.  C = NULL and G = I IN BITS (+1.0, +0.0, +0.0, +1.0): the map is the identity and Sigma is not passed over
 *      at all (the pending rows are still flushed), so every entry keeps its bits, NaN payloads and -0.0 included; step 1
 *      alone would turn a -0.0 beside a positive entry into +0.0 and spread a NaN over its block.
 * SIGMA IS NEVER SYMMETRISED: Sigma'[i][j] uses Sigma[i][j], never Sigma[j][i].  Sixteen bounds the rounded operations an
 * entry sees (4 products and 4 fused steps of step 1, 4 + 3 of step 2, 6 of step 3), so
 *   |Sigma' - J Sigma J^T|_ij <= gamma_16 ((|D| + |[C | 0]|) |Sigma| (|D| + |[C | 0]|)^T)_ij,  gamma_k = k u / (1 - k u), u = 2^-53.
 * (The tests hold the tighter form with |J| = |D + [C | 0]| entry by entry, which differs on the 3 x 3 pose block alone.)
 * On integer operands small enough for every intermediate to stay below 2^53 the result is exact in any order.
 * THE LAUNCHES.  A small launch (a thread per pair) snapshots the three pose rows and the three pose columns -- the only
 * walk down a column, 3 Na entries -- into the workspace and builds A, C^T and Bc^T as nine rows in the handle's [k][ld]
 * panel layout (two 6-row panels that share C^T).  The hot kernel makes one pass over Sigma[3:Na, 3:Na]: loads and stores
 * along rows, a 2 x 2 block is one lane's business, so the pass is in place with no staging copy of Sigma; tiles of
 * tile_rows x tile_cols states whose ORIGINS SIT ON ODD INDICES (3 + a tile_rows, 3 + b tile_cols), so no block straddles
 * two workgroups; the panel of a tile's columns sits in registers, the one of its rows comes through the scalar cache.  A
 * sibling launch writes the new pose rows and columns from the snapshot alone.  NO ATOMICS: A RUN REPEATS BIT FOR BIT, and
 * an entry's bits do not depend on N, on ld or on what lies outside the corner.  ekf_dense64_frame_launch_info reports the
 * tile sides in states and the workgroup size.  The workspace (19 ld + 4 doubles, 1.6 MB at N = 10003) comes from the
 * handle, allocated on first use; a failure there returns EKF_ERR_NOMEM and leaves the handle as it was.
 * ekf_dense64_reframe_landmarks transforms the state and Sigma together; the domain rules are those of the congruence, and a
 * mode other than the two below, or (FIXED) a dtheta, tx or ty that is not finite, returns EKF_ERR_INVALID.
 *   EKF_DENSE64_FRAME_FIXED: a known rigid transform.  theta' = theta + dtheta, NOT WRAPPED (as the reference's
 *     prediction()); q' = R(dtheta) q + t for the robot position and every landmark: x' = fl(fma(-s, y, fl(c x)) + tx),
 *     y' = fl(fma(c, y, fl(s x)) + ty).  G = R(dtheta) = [c, -s, s, c], C is absent.  c and s are taken ONCE ON THE HOST with
 *     the C library's cos and sin; the device applies them to the state in a small kernel.
 *   EKF_DENSE64_FRAME_ROBOT: the inverse pose composition -- the map in the robot's own frame, the old origin becomes the
 *     "pose"; dtheta, tx, ty are ignored.  With M = R(-theta), M' = dM/dtheta: theta' = -theta, p' = -M p,
 *     l_i' = M (l_i - p).  G = M; C: theta row [-2, 0, 0], position rows [-M' p | -2 M], landmark i [M' (l_i - p) | -M].
 *     G and C are built ON THE DEVICE from the handle's own state (the device's cos and sin): the pose never leaves the
 *     device.  The call is its own inverse up to rounding.  AFTERWARDS THE STATE IS
 *     NOT THE PARAMETERISATION ekf_dense64_predict_landmarks ASSUMES (the "pose" is the old origin seen from the robot):
 *     call it again before filtering on.
 *   terms_out (nullable, [4 + 3 Na] doubles): G [4] then C [Na][3] as they were used (FIXED: C comes back as zeros).  THE
 *   COVARIANCE RESULT IS, BIT FOR BIT, ekf_dense64_map_congruence WITH THOSE OPERANDS (FIXED: with C = NULL).
 * Out of scope: a transform with a covariance of its own, carrying the pending rows through the call.  (Joining two
 * handles is ekf_dense64_join_map, below.)
 * Synchronous, on the handle's stream.  elapsed_ms (nullable) = HIP-event time of the launches, the flush included. */
#define EKF_DENSE64_FRAME_FIXED 0
#define EKF_DENSE64_FRAME_ROBOT 1
ekf_status ekf_dense64_frame_launch_info(ekf_dense64_handle h, int* tile_rows, int* tile_cols, int* threads);
ekf_status ekf_dense64_map_congruence(ekf_dense64_handle h, const double* G /* [4] */, const double* C /* [Na][3], nullable */,
                                      double* elapsed_ms);
ekf_status ekf_dense64_reframe_landmarks(ekf_dense64_handle h, int mode, double dtheta, double tx, double ty,
                                         double* terms_out /* [4 + 3 Na], nullable */, double* elapsed_ms);

/* Map joining (Tardos, Neira, Newman, Leonard 2002): the map of a second handle appended to the map of the first, on the
 * device.  A local map B is built in a handle of its own (`src`), started at the robot's current pose with pose 0 and zero
 * pose covariance, so that every call on it costs Nb^2 and not N^2; the join then expresses its landmarks in the global frame
 * through the global robot pose, correlates them with the global map A (`dst`) through that pose's covariance, and replaces
 * the global pose by the composition of the two.  ekf_dense64_score_landmark_pairs / ekf_dense64_merge_landmarks then fuse
 * the landmarks both maps saw.  Instead of ekf_dense64_get_sigma of both handles, a host product and ekf_dense64_set of the
 * N^2 result, the join reads the source's corner once and writes the new corner and two rank-3 rectangles: 16 (Nb - 3)^2 +
 * 32 b (Na - 3) bytes and a few small launches.  Opt-in: no other entry point calls these or launches anything different
 * because they exist.
 * SETTING.  dst holds A: live dimension Na = 3 + 2 a, state (theta_A, p_A, l_1 .. l_a).  src holds B: live dimension
 * Nb = 3 + 2 b, b >= 0, state (theta_B, p_B, m_1 .. m_b), expressed in the frame of A's robot pose.  B MUST BE
 * STATISTICALLY INDEPENDENT OF A (the local map was started with pose 0 and zero pose covariance): THIS IS THE CALLER'S DUTY
 * AND IS NOT CHECKED.  With M = R(theta_A) = [c -s; s c] and M' = dM/dtheta = [-s -c; c -s] the joined state is
 *   pose' = (theta_A + theta_B, p_A + M p_B), THETA' IS NOT WRAPPED (as ekf_dense64_predict_landmarks and FRAME_FIXED do not);
 *   A's landmarks unchanged;  B's landmark j goes to dst's states Na + 2 j, Na + 2 j + 1 as p_A + M m_j,
 * and the new live dimension of dst is Na' = Na + 2 b.  b = 0 is legal: a pure pose composition.
 * OPERANDS.  G = M (row-major G[4]); D = blockdiag(1, G, ..., G), Nb x Nb, over the pairs (1, 2), (3, 4), ... as in the frame
 * calls; E, Nb x 3 row-major: row 0 = [1, 0, 0], rows (1, 2) = [M' p_B | I_2], rows (3 + 2 j, 4 + 2 j) = [M' m_j | I_2].
 * E IS A GENERAL OPERAND: every entry is multiplied through, the zeros and ones are not skipped.  From dst's Sigma ON ENTRY
 * (after the flush): P = Sigma_A[0:3, :] (the three pose rows, read along rows), Pc = Sigma_A[:, 0:3] (the three pose
 * columns), Sigma_pp the 3 x 3 corner.
 * DEFINITION, every operation in IEEE binary64, round to nearest even, each rounded on its own (fl) unless it is written as
 * a fused multiply-add fma(a, b, c) = fl(a b + c).  SIGMA IS NEVER SYMMETRISED, neither A's nor B's:
 *   1. Z = D Sigma_B D^T: exactly step 1 of ekf_dense64_map_congruence on src's corner -- the same four products and four
 *      fused steps per 2 x 2 block, the same one-sided products on row 0 and column 0.
 *   2. W = E Sigma_pp (Nb x 3): W[k][l] = fl(E[k][0] * Sigma_pp[0][l]), then W[k][l] = fma(E[k][t], Sigma_pp[t][l], W[k][l])
 *      for t = 1, 2.
 *   3. Y = Z + W E^T: acc = Z[i][j]; acc = fma(W[i][l], E[j][l], acc) for l = 0, 1, 2.
 *   4. The cross terms.  X_rows (Nb x Na): X_rows[k][j] = fl(E[k][0] * P[0][j]), then fma(E[k][l], P[l][j], .) for l = 1, 2.
 *      X_cols (Na x Nb): X_cols[i][k] = fl(Pc[i][0] * E[k][0]), then fma(Pc[i][l], E[k][l], .) for l = 1, 2.
 *   5. Placement, with iota: src index 0, 1, 2 -> 0, 1, 2 and 3 + t -> Na + t:
 *        Sigma'[iota(i)][iota(j)] = Y[i][j];
 *        Sigma'[iota(k)][j] = X_rows[k][j] for 3 <= j < Na;      Sigma'[i][iota(k)] = X_cols[i][k] for 3 <= i < Na;
 *        SIGMA'[3:Na, 3:Na] IS NOT TOUCHED: NOT READ, NOT WRITTEN.  Nothing at a dst index >= Na' and nothing at a src index
 *        >= Nb is read or written: loads and stores are masked element by element, a pair is inside or outside as a whole.
 * AN ENTRY OF Y SEES 14 ROUNDED OPERATIONS (4 products and 4 fused steps of step 1, 3 of step 2, 3 of step 3), A CROSS ENTRY
 * 3.  With J the Na' x (Na + Nb) Jacobian of the joined state on (A, B) -- the identity on A's landmarks, [E | 0 | D] in the
 * rows iota(.) -- and Sigma = blockdiag(Sigma_A, Sigma_B):
 *   |Sigma' - J Sigma J^T|_ij <= gamma_14 (|J| |Sigma| |J|^T)_ij,  gamma_k = k u / (1 - k u), u = 2^-53
 * (gamma_3 on the two rectangles and on the pose rows and columns below Na).  On integer operands small enough for every
 * intermediate to stay below 2^53 the result is exact in any order.
 * ekf_dense64_join_congruence is the kernels' own entry point: Sigma only, with the caller's G and E.  It sets dst's live
 * dimension to Na' and TOUCHES NEITHER STATE VECTOR.
 * ekf_dense64_join_map builds G and E ON THE DEVICE from dst's own heading (the device's cos and sin, as FRAME_ROBOT does)
 * and src's state, transforms the state with FRAME_FIXED's expressions -- x' = fl(fma(-s, y, fl(c x)) + p_Ax),
 * y' = fl(fma(c, y, fl(s x)) + p_Ay), theta' = fl(theta_A + theta_B) -- and runs the same covariance launches.  terms_out
 * (nullable, [4 + 3 Nb] doubles): G [4] then E [Nb][3] as they were used.  ITS COVARIANCE RESULT IS, BIT FOR BIT,
 * ekf_dense64_join_congruence WITH THOSE OPERANDS.
 * REFUSALS.  Every refusal returns EKF_ERR_INVALID before the device is looked at and changes nothing in either handle, the
 * pending rows and an open region included.  THE CHECKS COME IN THIS ORDER: (1) NULL dst; (2) NULL src; (3) dst == src;
 * (4) the handles live on different devices; (5) dst's live and src's live both odd and >= 3; (6) Na + 2 b <= dst's N;
 * (7) NULL G or E (ekf_dense64_join_congruence only).
 * PENDING ROWS, REGIONS, STREAMS.  dst needs Sigma in memory, so it FLUSHES ITS PENDING ROWS FIRST, carry or not, after the
 * checks and inside the timed region; an open region on dst is ended first, like every call outside a region's terms.  src
 * is brought to Sigma in memory as ekf_dense64_get_sigma would: its pending rows are flushed and an open region is ended,
 * on src's own stream; an event recorded there is waited on by dst's stream.  OTHERWISE SRC IS READ-ONLY: its Sigma values,
 * its state and its live dimension are unchanged, and the caller can go on using it or reset it.  All join launches run on
 * dst's stream, which is synchronised before the call returns.  dst's factor snapshot stays as taken (ekf_dense64_factor).
 * THE LAUNCHES.  A small launch snapshots P and Pc of dst -- the only walk down a column of dst, 3 Na entries -- and builds W.
 * The hot kernel makes one pass over src's Sigma[3:Nb, 3:Nb] in the frame pass's shape: tiles of tile_rows x tile_cols
 * states whose ORIGINS SIT ON ODD INDICES, a 2 x 2 block per lane, loads along src's rows issued ahead of use, E of a tile's
 * columns in registers, W of its rows through the scalar cache, no LDS; it stores to dst at the shifted origin with dst's
 * leading dimension, so it is out of place and has no hazard.  One launch per rectangle writes X_rows[3:, 3:Na] and
 * X_cols[3:Na, 3:] along rows, and a sibling of the snapshot writes the three new pose rows and columns over [0, Na').
 * (join_map: one small launch in front for the terms and the state; the new pose goes through a staging slot and is copied
 * over behind the launches, so every thread reads the old pose.)  NO ATOMICS, NO REDUCTIONS: A RUN REPEATS BIT FOR BIT, and an entry's bits depend on neither handle's
 * N or ld.  ekf_dense64_join_launch_info reports the hot kernel's tile sides in states and its workgroup size.  The workspace
 * (6 ld + 6 Nb + 8 doubles) comes from DST's ledger, allocated on first use and grown with Nb; a failure there returns
 * EKF_ERR_NOMEM and leaves both handles as they were.
 * Out of scope: joining across devices, carrying the pending rows through the join, a source pose with a prior correlation
 * to A.  Synchronous.  elapsed_ms (nullable) = HIP-event time on dst's stream, both flushes included;
 * ekf_dense64_join_congruence: the uploads of G and E are queued in front of it and are not (as ekf_dense64_map_congruence's). */
ekf_status ekf_dense64_join_launch_info(ekf_dense64_handle h, int* tile_rows, int* tile_cols, int* threads);
ekf_status ekf_dense64_join_congruence(ekf_dense64_handle dst, ekf_dense64_handle src, const double* G /* [4] */,
                                       const double* E /* [Nb][3] */, double* elapsed_ms);
ekf_status ekf_dense64_join_map(ekf_dense64_handle dst, ekf_dense64_handle src, double* terms_out /* [4 + 3 Nb], nullable */,
                                double* elapsed_ms);

/* A map, or a submap, copied into a second handle: the inverse of the join, and the only copy of a dense filter that does
 * not go through the host.  Three uses, one operation: a SNAPSHOT before an ambiguous association or a merge (keep == NULL:
 * a clone; run both branches, keep one, or extract back to restore); a SUBMAP cut out of the global map, the pose plus a
 * chosen list of landmarks -- the EKF's marginalisation is the deletion of rows and columns, so the submap is exact; and
 * PRUNING many landmarks at once, k of b kept in one out-of-place pass instead of one swap_blocks / init_block / set_live
 * per landmark.
 * THE DEFINITION.  src has the live dimension Nb = 3 + 2 b.  keep [k]: landmarks of src in [0, b), no repeats, any order;
 * keep == NULL is the identity list of all b (k is then b, or -1 for "whatever b is"); k = 0 copies the pose alone.  With
 *   iota(0, 1, 2) = 0, 1, 2,   iota(3 + 2 t + c) = 3 + 2 keep[t] + c  (c = 0, 1),   Nd = 3 + 2 k:
 *   Sigma_dst[i][j] takes the bits of Sigma_src[iota(i)][iota(j)],  x_dst[i] the bits of x_src[iota(i)],  i, j < Nd,
 * and dst's live dimension becomes Nd.  A PURE COPY: no arithmetic, so a NaN keeps its payload, a zero its sign and a Sigma
 * that is never symmetrised its asymmetry.  Nothing at a dst index >= Nd is read or written, nothing at a src index >= Nb is
 * read, whatever either handle's N and ld are.
 * PENDING ROWS ARE CARRIED, NOT APPLIED.  A pending row is linear in the same index, so when src has p rows pending
 * (ekf_dense64_pending) dst has the same p afterwards: K_dst[q][i] = K_src[q][iota(i)] and T likewise, zero from Nd up to the
 * width the calls of that live width keep zero (Nd rounded up to 128, at most ld: ekf_dense64_set_live's convention).  A
 * snapshot in mid-tick therefore costs no flush, and Sigma_cur of dst (ekf_dense64_get_sigma_block under carry) is Sigma_cur
 * of src at iota x iota bit for bit.  dst's panels come from its ledger if it has none.  SRC IS UNCHANGED BIT FOR BIT: Sigma,
 * state, pending rows, their count and the live dimension -- except that an open region on src is ended first, on src's
 * stream, like every call outside a region's terms (which applies the rows pending inside it: p is then 0).  DST IS THE ONE
 * OVERWRITTEN: an open region on it is ended and its own pending rows are applied first, as the join does, inside the timed
 * region; it costs nothing when nothing is pending.  dst's carry flag, factor snapshot and tuning stay as they are.
 * REFUSALS.  Every refusal returns EKF_ERR_INVALID before the device is looked at and changes nothing in either handle, the
 * pending rows and an open region included.  THE CHECKS COME IN THIS ORDER: (1) NULL dst; (2) NULL src; (3) dst == src;
 * (4) the handles live on different devices; (5) src's live dimension not odd or below 3; (6) k < 0, or keep == NULL with k
 * neither b nor -1; (7) an index of keep outside [0, b); (8) an index of keep repeated; (9) 3 + 2 k > dst's N.  A failed
 * ledger allocation (the list's workspace, 4 (65 ceil(k / 64) + 4) bytes, or the panels) returns EKF_ERR_NOMEM and leaves
 * both handles as they were.
 * STREAMS as the join's: src's region end runs on src's own stream, an event recorded there is waited on by dst's stream,
 * every extract launch runs on dst's stream, which is synchronised before the call returns.
 * THE LAUNCHES.  The list goes up once, with one flag per column tile found while it is validated.  The hot kernel makes one
 * pass over dst's Sigma[3:Nd, 3:Nd] in the frame and join passes' shape: tiles of tile_rows x tile_cols states whose ORIGINS
 * SIT ON ODD INDICES, a 2 x 2 block per lane, 16-byte loads along src's rows all issued before the first store, stores along
 * dst's rows, no LDS.  A tile's row landmarks are wave-uniform and come through the scalar cache.  A COLUMN TILE WHOSE
 * LANDMARKS ARE A CONTIGUOUS ASCENDING RUN OF SRC (a clone, a prefix, any list of runs of 64 on tile boundaries) takes its
 * columns from the tile's first landmark plus the lane: a wave's load is 1 KiB of one src row, the join kernel's access.  Any
 * other tile reads its landmarks from the list: the same result from sixty-four separate 16-byte pieces of the row.  A
 * sibling launch copies the three pose rows and columns, the 3 x 3 corner and the Nd states; one more, when p > 0, the
 * p x Nd rows of both panels.  NO ATOMICS, NO REDUCTIONS: A RUN REPEATS BIT FOR BIT.  ekf_dense64_extract_launch_info reports
 * the hot kernel's tile sides in states and its workgroup size.  Bytes: 16 Nd^2 (8 read, 8 written) plus 32 p Nd.
 * Out of scope: extraction in place (dst == src), across devices, and a general state list that breaks landmark pairs.
 * Synchronous.  elapsed_ms (nullable) = HIP-event time on dst's stream, dst's own flush and region end included; the upload
 * of the list is queued in front of it and is not. */
ekf_status ekf_dense64_extract_launch_info(ekf_dense64_handle h, int* tile_rows, int* tile_cols, int* threads);
ekf_status ekf_dense64_extract_map(ekf_dense64_handle dst, ekf_dense64_handle src,
                                   int k, const int* keep /* [k] landmarks of src, any order; NULL = all, in order */,
                                   double* elapsed_ms);

/* Block readout and state slices: what a caller that publishes the 3 x 3 pose covariance every tick, or wraps the heading
 * after a correction, needs instead of the N^2 doubles of ekf_dense64_get_sigma and the N of get_state / set_state.
 * ekf_dense64_get_sigma_block: out[a][c] = Sigma[rows[a]][cols[c]], nr x nc row-major; one gather launch into a buffer
 * allocated with the handle and one copy.  nr, nc >= 1, nr * nc <= EKF_DENSE64_READ_MAX, indices in [0, N), repeats
 * allowed, any order.  Read-only.
 * ekf_dense64_get_state_block / ekf_dense64_set_state_block: copies of `count` doubles from / to state[first ..],
 * 1 <= count, 0 <= first, first + count <= N; nothing else of the state is touched.
 * A NULL handle (checked first), a NULL array, a bad count or range or an index outside [0, N) return EKF_ERR_INVALID
 * before the device is looked at.  Synchronous, on the handle's stream. */
#define EKF_DENSE64_READ_MAX 65536
ekf_status ekf_dense64_get_sigma_block(ekf_dense64_handle h, int nr, const int* rows, int nc, const int* cols,
                                       double* out /* nr x nc */);
ekf_status ekf_dense64_get_state_block(ekf_dense64_handle h, int first, int count, double* out);
ekf_status ekf_dense64_set_state_block(ekf_dense64_handle h, int first, int count, const double* x);

/* ---- laser-scan front end: rigid2d::CircleFitting, batched ----------
 * std::vector<Vector2D> approxCirclePositions(std::vector<double> ranges)
 *                                          circle_fitting.hpp:27, circle_fitting.cpp:298-304
 * = clusteringRanges (:11-90) + circleRegression (:104-232) + classifyCircle (:234-296): the producer
 * of the `measures` argument of data_association (nuslam/src/landmarks.cpp:141 ->
 * unknown_data_assoc.cpp:309-320).  S scans of n_beams ranges each (beam i at angle 2*pi*i/n_beams):
 *   centres [S][max_out][2], radii [S][max_out], counts [S] (circles kept per scan, <= max_out);
 *   all_clusters (nullable) [S][128][4] = {x, y, r, is_circle} of EVERY cluster, n_clusters (nullable) [S].
 * n_beams <= 1024.  A scan without any cluster (undefined behaviour in the reference, :54) gives 0. */
ekf_status ekf_circle_fit_scans(int device, const double* ranges, int S, int n_beams, int max_out,
                                double* centres, double* radii, int* counts, double* all_clusters,
                                int* n_clusters);

#ifdef __cplusplus
}
#endif
#endif /* EKFSLAM_H */
