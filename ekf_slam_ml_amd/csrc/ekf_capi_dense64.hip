// ekf_capi_dense64.hip -- C ABI of include/ekfslam.h, what the fp64 dense handle has beyond the propagation it shares with
// the fp32 one (ekf_capi_dense.hip): a state vector, the dense measurement update (ekf_dense64_correct.hip), the read-only
// scoring of candidates (ekf_dense64_score.hip), the block-structured prediction (ekf_dense64_block.hip), the update and
// scoring for a Jacobian given by its non-zero columns (ekf_dense64_sparse.hip), the (re)initialisation of a block of states
// and the block readout (ekf_dense64_init.hip), the exchange of two blocks (ekf_dense64_swap.hip), the landmark front end
// (ekf_dense64_landmarks.hip), the reference's prediction() and measurement() on that state (ekf_dense64_model.hip), the
// scan of all landmark pairs for duplicates and their merge (ekf_dense64_pairs.hip), the health check of the live corner and its
// exact symmetrisation (ekf_dense64_health.hip), its Cholesky factor with the substitution against it
// (ekf_dense64_factor.hip), the Joseph form of the sparse update with per-state gain weights (ekf_dense64_joseph.hip), the
// map re-expressed in another frame (ekf_dense64_frame.hip), a second handle's map joined onto it (ekf_dense64_join.hip), a map
// or a submap copied into a second handle (ekf_dense64_extract.hip), what observing each landmark would gain
// (ekf_dense64_value.hip), a laser scan cast against the map for evidence on each landmark (ekf_dense64_evidence.hip), and
// the deferred form of the sparse update: pending rows of K and T that the sparse calls
// read through and every other call that touches Sigma applies first (flush_pending) -- unless the caller lets
// propagate_block, init_block, swap_blocks and the block readout carry them (ekf_dense64_set_carry, ekf_dense64_carry.hip).
// The structured calls run at the handle's LIVE dimension (ekf_dense64_set_live, N by default): every launch of theirs is
// cut for it, and nothing at an index from it on is read or written; ekf_dense64_coupling (ekf_dense64_live.hip) measures
// what ties the live corner to the rest.  Where an operand sits in its buffer is ekf_dense64_layout.hpp's business; the
// entry points see the typed views of ekf_dense_handle.hpp only.
#include "ekf_dense64_evidence.hpp"
#include "ekf_dense64_jcbb.hpp"
#include "ekf_dense_handle.hpp"

using namespace ekfrt;

ekf_status ekf_dense64_s::created() {
    HIPC(ekf::dense64_correct_prepare());
    HIPC(ekf::dense64_block_prepare());
    HIPC(ekf::dense64_sparse_prepare());
    HIPC(ekf::dense64_joseph_prepare());
    HIPC(ekf::dense64_init_prepare());
    HIPC(ekf::dense64_region_prepare());
    live = N;
    pl_full = pl_live = ekf::dense64_correct_plan(N, ld);
    const char *fn = "ekf_dense64_create", *what = "the operand buffers";
    EKFC(mem.replace_group({target_bytes(&x, sizeof(double) * ld, Fill::kZero), target_bytes(&corr_in, L::corr_in_layout(ld).bytes, Fill::kZero),
                            target_bytes(&corr_out, L::corr_out_layout().bytes), target_bytes(&blk_in, L::blk_in_layout().bytes),
                            target_bytes(&ini_in, L::ini_in_layout().bytes), target_bytes(&rd_buf, L::rd_buf_layout().bytes)}, fn, what));
    if (pl_full.ws_doubles > (size_t)ld * ld) EKFC(mem.alloc(&ws_own, pl_full.ws_doubles, Fill::kNone, fn, what));
    return EKF_OK;
}

void ekf_dense64_s::destroying() { scan_up.release(); }

namespace {

constexpr int kMaxM = ekf::kDense64MaxM, kMaxR = ekf::kDense64MaxR, kMaxS = ekf::kDense64MaxS;
constexpr int kMaxP = ekf::kDense64PendingMaxRows, kReadMax = ekf::kDense64ReadMax;
constexpr int kScoreRows = ekf::kDense64ScoreMaxRows, kSparseRows = ekf::kDense64ScoreSparseMaxRows;

// finish_timed of a correction: corr_out (nis | verdict) comes back in one copy; *verdict: 0 = applied, 1 = S singular.
// also, also2: further copies behind the same synchronisation (a null dst is skipped).
ekf_status finish_correction(ekf_dense64_s* d, double* elapsed_ms, double* nis, int* verdict, const CopyBack& also = {},
                             const CopyBack& also2 = {}) {
    double out[2] = {0.0, 0.0};
    EKFC(finish_timed(d, elapsed_ms, {{out, d->corr_out, sizeof(out)}, also, also2}));
    *nis = out[0];
    std::memcpy(verdict, &out[1], sizeof(int));
    return EKF_OK;
}

// every row of cols [rows][s]: indices in [0, N), no index twice
bool index_lists_ok(std::vector<int>& stamp, int N, int rows, int s, const int* cols) {
    stamp.assign(N, 0);
    for (int j = 0; j < rows; j++)
        for (int k = 0; k < s; k++) {
            const int c = cols[(size_t)j * s + k];
            if (c < 0 || c >= N || stamp[c] == j + 1) return false;
            stamp[c] = j + 1;
        }
    return true;
}

// ---- a Jacobian given by its s non-zero columns ---------------------------------------------------------------------------
// One sparse correction: cols, Hc, R, nu go up into the (otherwise unused) operand buffer of the dense correction
// (CorrSparseLayout), the verdict and nis come back in one copy.  Eager: the pending rows are applied first, four launches.
// Deferred: three launches (no pass over Sigma) unless the m new rows do not fit; K and T stay in the pending panels, which
// the first call allocates.
// The public entry point is checks | pend_reserve | uploads | e0 | correct_sparse_launch | correct_sparse_finish; a caller
// that builds the operands on the device (the landmark front end) writes them through the same view and runs the last two.
ekf_status pend_reserve(ekf_dense64_s* d, const char* fn) {
    return d->pend.reserve(d->mem, L::pend_layout(d->ld).bytes, true, fn, "the pending panels");
}

// the launches of one correction on operands that sit in the operand buffer; behind e0.  joseph_w (eager only): the Joseph
// form, with the weights that sit in the workspace (dense64_joseph_ws) or all 1
enum class Joseph { kNo, kUnweighted, kWeighted };
void correct_sparse_launch(ekf_dense64_s* d, bool deferred, int m, int s, bool have_nu, Joseph joseph = Joseph::kNo) {
    const CorrSparseView in = view(d->corr_in, L::corr_sparse_layout(d->ld));
    const CorrOutView out = view(d->corr_out, L::corr_out_layout());
    const double* dnu = have_nu ? in.nu : nullptr;
    if (!deferred || d->pend_rows + m > kMaxP) d->flush_pending();   // deferred: only when there is no room for m more rows
    const PendView p = d->panels();
    const int p0 = d->pend_rows;   // (behind the flush) where a deferred call leaves its rows of K^T
    if (joseph != Joseph::kNo)
        ekf::launch_dense64_correct_sparse_joseph(
            d->pl_live, d->S, d->x, d->workspace(), in.cols, in.Hc, in.R, dnu,
            joseph == Joseph::kWeighted ? ekf::dense64_joseph_ws(d->pl_live, d->workspace()).w : nullptr, m, s, out.nis,
            out.verdict, d->stream);
    else if (deferred)
        ekf::launch_dense64_correct_deferred(d->pl_live, d->S, d->x, d->workspace(), p.K, p.T, d->pend_rows, in.cols, in.Hc,
                                             in.R, dnu, m, s, out.nis, out.verdict, d->stream);
    else
        ekf::launch_dense64_correct_sparse(d->pl_live, d->S, d->x, d->workspace(), in.cols, in.Hc, in.R, dnu, m, s, out.nis,
                                           out.verdict, d->stream);
    if (d->region_on)   // the accumulators take the gain, S^-1 and nu the live call used (no Joseph form inside a region)
        ekf::launch_dense64_region_correct(d->region_pl, d->region_mem.acc,
                                           deferred ? p.K + (size_t)p0 * d->ld : d->workspace() + d->pl_live.off_Kt, d->ld,
                                           d->workspace() + d->pl_live.off_Sinv, in.cols, in.Hc, dnu, m, s, out.verdict,
                                           d->stream);
}

// the one synchronisation of a correction, its verdict, the count of the pending rows
ekf_status correct_sparse_finish(ekf_dense64_s* d, const char* fn, bool deferred, int m, double* nis_out,
                                 double* elapsed_ms, const CopyBack& also = {}, const CopyBack& also2 = {}) {
    double nis = 0.0;
    int verdict = 0;
    EKFC(finish_correction(d, elapsed_ms, &nis, &verdict, also, also2));
    if (verdict != 0)
        return fail(EKF_ERR_STATE, std::string(fn) + ": H Sigma H^T + R is singular or not finite (zero or non-finite pivot); " +
                                       (deferred ? "state, Sigma and the pending rows are unchanged"
                                                 : "state and Sigma are unchanged"));
    if (deferred) d->pend_rows += m;
    if (d->region_on) d->region_corrections++;
    if (nis_out) *nis_out = nis;
    return EKF_OK;
}

ekf_status dense64_correct_sparse(ekf_dense64_s* d, bool deferred, int m, int s, const int* cols, const double* Hc,
                                  const double* R, const double* nu, double* nis_out, double* elapsed_ms) {
    const std::string fn = deferred ? "ekf_dense64_correct_sparse_deferred" : "ekf_dense64_correct_sparse";
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    if (!cols || !Hc || !R || m < 1 || m > kMaxM || m > d->live || s < 1 || s > kMaxS || s > d->live || (nis_out && !nu))
        return fail(EKF_ERR_INVALID, fn + ": bad argument");
    if (!index_lists_ok(d->host_stamp, d->live, 1, s, cols))
        return fail(EKF_ERR_INVALID, fn + ": cols must hold distinct indices in [0, N), below the live dimension");
    HIPC(hipSetDevice(d->device));
    if (deferred) EKFC(pend_reserve(d, fn.c_str()));
    const CorrSparseView in = view(d->corr_in, L::corr_sparse_layout(d->ld));
    HIPC(hipMemcpyAsync(in.Hc, Hc, sizeof(double) * m * s, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(in.cols, cols, sizeof(int) * s, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(in.R, R, sizeof(double) * m * m, hipMemcpyHostToDevice, d->stream));
    if (nu) HIPC(hipMemcpyAsync(in.nu, nu, sizeof(double) * m, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    correct_sparse_launch(d, deferred, m, s, nu != nullptr);
    return correct_sparse_finish(d, fn.c_str(), deferred, m, nis_out, elapsed_ms);
}

// The Joseph form: ekf_dense64_correct_sparse's checks with the cap on m at 32, then the weights' host scan (which also
// counts the tiles the pass will skip); the weights go up with the operands, the pending rows are applied inside the timed
// region, and the verdict and nis come back as they do there.
constexpr int kJosephMaxM = ekf::kDense64JosephMaxM;
static_assert(kJosephMaxM == EKF_DENSE64_JOSEPH_MAX_M, "ekfslam.h and ekf_dense.hpp");

ekf_status dense64_correct_sparse_joseph(ekf_dense64_s* d, int m, int s, const int* cols, const double* Hc, const double* R,
                                         const double* nu, const double* gain_w, double* nis_out, long long* tiles_skipped,
                                         double* elapsed_ms) {
    const std::string fn = "ekf_dense64_correct_sparse_joseph";
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!cols || !Hc || !R || m < 1 || m > kJosephMaxM || m > d->live || s < 1 || s > kMaxS || s > d->live || (nis_out && !nu))
        return fail(EKF_ERR_INVALID, fn + ": bad argument (1 <= m <= 32)");
    if (!index_lists_ok(d->host_stamp, d->live, 1, s, cols))
        return fail(EKF_ERR_INVALID, fn + ": cols must hold distinct indices in [0, N), below the live dimension");
    const int Na = d->live, tr = ekf::kDense64JosephTileRows, tc = ekf::kDense64JosephTileCols;
    long long skipped = 0;
    if (gain_w) {
        for (int i = 0; i < Na; i++)
            if (!(gain_w[i] >= 0.0 && gain_w[i] <= 1.0))   // (a NaN fails both comparisons)
                return fail(EKF_ERR_INVALID, fn + ": every gain weight below the live dimension must be finite and in [0, 1]");
        auto idle = [&](int side) {   // groups of `side` states without a w != 0
            long long n = 0;
            for (int i0 = 0; i0 < Na; i0 += side) {
                bool any = false;
                for (int i = i0; i < std::min(Na, i0 + side) && !any; i++) any = gain_w[i] != 0.0;
                n += any ? 0 : 1;
            }
            return n;
        };
        skipped = idle(tr) * idle(tc);
    }
    HIPC(hipSetDevice(d->device));
    const CorrSparseView in = view(d->corr_in, L::corr_sparse_layout(d->ld));
    HIPC(hipMemcpyAsync(in.Hc, Hc, sizeof(double) * m * s, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(in.cols, cols, sizeof(int) * s, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(in.R, R, sizeof(double) * m * m, hipMemcpyHostToDevice, d->stream));
    if (nu) HIPC(hipMemcpyAsync(in.nu, nu, sizeof(double) * m, hipMemcpyHostToDevice, d->stream));
    if (gain_w)
        HIPC(hipMemcpyAsync(ekf::dense64_joseph_ws(d->pl_live, d->workspace()).w, gain_w, sizeof(double) * Na,
                            hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    correct_sparse_launch(d, false, m, s, nu != nullptr, gain_w ? Joseph::kWeighted : Joseph::kUnweighted);
    EKFC(correct_sparse_finish(d, fn.c_str(), false, m, nis_out, elapsed_ms));
    if (tiles_skipped) *tiles_skipped = skipped;
    return EKF_OK;
}

// Sparse scoring of J candidates: the operands go up into one buffer (SpsLayout), one launch, the outputs come straight back
// into the caller's arrays.
// The public entry point is checks | sps_layout | sps_reserve | uploads | e0 | score_sparse_launch | copies back; a caller
// that builds the operands on the device (the landmark front end) writes them through the same view and launches the same.
ekf_status sps_reserve(ekf_dense64_s* d, size_t need, const char* fn) {
    return d->sps.reserve(d->mem, need, false, fn, "the candidates' buffer");
}
// the one launch on operands that sit in the buffer: eager, or read-through as rows are pending
void score_sparse_launch(ekf_dense64_s* d, const SpsView& v, int J, int m, int s, bool r_shared, bool have_nu,
                         bool want_nis) {
    const PendView p = d->panels();   // (null before the first deferred call)
    ekf::launch_dense64_score_sparse(d->S, p.K, d->pend_rows ? p.T : nullptr, d->pend_rows, v.cols, v.Hc, v.R,
                                     r_shared ? 1 : 0, have_nu ? v.nu : nullptr, J, m, s, d->ld, want_nis ? v.nis : nullptr,
                                     v.S, v.flag, nullptr, d->stream);
}

// ---- (re)initialisation of a block of states -----------------------------------------------------------------------------
// the launches on operands that sit in ini_in (the public call after its uploads, the landmark front end after
// k_dlm_decide): the pending rows carried or applied, then the one launch; behind e0
// W, xb: on the device (ini_in's own, or the stacked ones of the joint association), null as the public call defines
void init_block_launch(ekf_dense64_s* d, int first, int r, int s, const double* W, const double* xb) {
    const IniInView in = view(d->ini_in, L::ini_in_layout());
    d->carry_or_flush([&](const PendView& p) {
        ekf::launch_dense64_panel_map(p.K, p.T, d->pend_rows, in.G, s > 0 ? in.cols : nullptr, d->ld, first, r, s, d->stream);
    });
    ekf::launch_dense64_init(d->S, d->x, in.cols, in.G, W, xb, d->live, d->ld, first, r, s, d->stream);
    d->region_row_map(in.G, s > 0 ? in.cols : nullptr, first, r, s);
}

ekf_status dense64_state_block(const char* name, ekf_dense64_s* d, int first, int count, double* out, const double* x) {
    if (!d) return fail(EKF_ERR_INVALID, std::string(name) + ": null handle");
    if ((!out && !x) || count < 1 || first < 0 || count > d->N || first > d->N - count)
        return fail(EKF_ERR_INVALID, std::string(name) + ": bad argument");
    if (first + count > d->live) d->leave_region();   // (live < N inside a region: the block reaches beyond it)
    HIPC(hipSetDevice(d->device));
    if (out) HIPC(hipMemcpyAsync(out, d->x + first, sizeof(double) * count, hipMemcpyDeviceToHost, d->stream));
    else HIPC(hipMemcpyAsync(d->x + first, x, sizeof(double) * count, hipMemcpyHostToDevice, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}

ekf::Params landmark_params(const ekf_params* params) {
    ekf_params p;
    ekf_default_params(&p);
    if (params) p = *params;
    return ekf::Params{p.sigma0_landmark, p.q_pose, p.r_meas, p.gate_new, p.gate_update, p.straight_eps};
}


// ---- one laser scan -> circles (ekf_dense64_scan.hip) ---------------------------------------------------------------------
// The ranges go up through a slot of the pinned ring, one launch on the handle's stream, and the record {circles kept,
// clusters, centres, radii} (and every cluster's row when asked for) comes down into d->scan_rec behind ONE synchronisation.
// The device buffer and the ring are reserved by the first call; a later call allocates nothing.  Read-only on the filter.
constexpr int kScanBeams = ekf::kDense64ScanMaxBeams, kScanClusters = ekf::kDense64ScanMaxClusters;

struct ScanRecord { int count, n_clusters; const double *centres, *radii, *all; };   // views of d->scan_rec

ekf_status scan_fit(ekf_dense64_s* d, const char* fn, const double* ranges, int n_beams, int max_out, bool want_all,
                    double* elapsed_ms, ScanRecord* rec) {
    const L::ScanLayout l = L::scan_layout();
    if (!d->scan.p) {
        for (Staging& sg : d->scan_up.slot) EKFC(sg.reserve(sizeof(double) * kScanBeams));
        d->scan_rec.assign((l.bytes - l.head) / sizeof(double), 0.0);
    }
    EKFC(d->scan.reserve(d->mem, l.bytes, true, fn, "the scan buffer"));
    const ScanView v = view(d->scan.p, l);
    Staging& sg = d->scan_up.acquire();
    EKFC(sg.wait());
    std::memcpy(sg.host, ranges, sizeof(double) * n_beams);
    HIPC(hipMemcpyAsync(v.ranges, sg.host, sizeof(double) * n_beams, hipMemcpyHostToDevice, d->stream));
    EKFC(sg.mark(d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->finish_leave();   // (a region that is being left ends here)
    ekf::launch_dense64_scan_circles(v.ranges, n_beams, max_out, v.head, v.centres, v.radii, v.all, d->stream);
    char* host = reinterpret_cast<char*>(d->scan_rec.data());
    EKFC(finish_timed(d, elapsed_ms, {{host, v.head, l.record_bytes},
                                      {want_all ? host + (l.all - l.head) : nullptr, v.all, l.bytes - l.all}}));
    const int* head = reinterpret_cast<const int*>(host);
    if (head[0] < 0 || head[0] > max_out || head[1] < 0 || head[1] > kScanClusters)
        return fail(EKF_ERR_HIP, std::string(fn) + ": the circle kernel left an impossible record");
    *rec = ScanRecord{head[0], head[1], reinterpret_cast<const double*>(host + (l.centres - l.head)),
                      reinterpret_cast<const double*>(host + (l.radii - l.head)),
                      reinterpret_cast<const double*>(host + (l.all - l.head))};
    return EKF_OK;
}

// the legs of a call with several synchronisations: behind each one the time between its events (0 when it failed before
// reading them) joins the total, which *out (nullable; on entry the time of what ran before) follows
struct LegTimer {
    double* out;
    double total, ms = 0.0;
    explicit LegTimer(double* elapsed_ms) : out(elapsed_ms), total(elapsed_ms ? *elapsed_ms : 0.0) {}
    double* pms() { return out ? &ms : nullptr; }
    ekf_status operator()(ekf_status st) { total += ms; ms = 0.0; if (out) *out = total; return st; }
};

// ---- data_association (:278-402), shared by ekf_dense64_associate_landmarks and ekf_dense64_associate_scan -----------------
// the flags of the landmark front end: `allowed` is what the call knows; the Joseph form is eager only
ekf_status lm_flags_ok(const std::string& fn, unsigned flags, unsigned allowed) {
    if (flags & ~allowed) return fail(EKF_ERR_INVALID, fn + ": unknown flag bits");
    if ((flags & EKF_DENSE64_LM_JOSEPH) && (flags & EKF_DENSE64_LM_DEFERRED))
        return fail(EKF_ERR_INVALID, fn + ": EKF_DENSE64_LM_JOSEPH is an eager form and does not combine with "
                                          "EKF_DENSE64_LM_DEFERRED");
    return EKF_OK;
}
Joseph lm_joseph(unsigned flags) { return (flags & EKF_DENSE64_LM_JOSEPH) ? Joseph::kUnweighted : Joseph::kNo; }

// what the loop below needs in memory
ekf_status associate_reserve(ekf_dense64_s* d, const char* fnc, int n_max, bool deferred) {
    EKFC(d->lm_rec.reserve(d->mem, sizeof(ekf::Dense64LmRecord), false, fnc, "the decision record"));
    if (deferred) EKFC(pend_reserve(d, fnc));
    // the scoring buffer once, for the full map: a map that is being discovered must not pay a hipMalloc and a hipFree
    // (a device synchronisation) per new landmark
    if (n_max > 0) EKFC(sps_reserve(d, L::sps_layout(n_max, 2, 5, true, false).bytes, fnc));
    return EKF_OK;
}

// J readings in order.  Per reading: [terms | score | decide] and the 32-byte record back (the first synchronisation); then,
// as the record says, [init_block] [terms of the winner, wrapped | correction | heading wrap] and the correction's own
// synchronisation.  Nothing of the state comes down and no candidate array goes up.  *elapsed_ms (nullable) holds the time
// of what ran before (0, or the circle fit's) and the legs of this loop join it.
ekf_status associate_readings(ekf_dense64_s* d, const char* fnc, const ekf::Params& p, int J, const double* meas_xy, int n_max,
                              int* known, unsigned flags, int* assoc_out, double* best_out, double* elapsed_ms) {
    const std::string fn = fnc;
    const bool deferred = (flags & EKF_DENSE64_LM_DEFERRED) != 0;
    ekf::Dense64LmRecord* drec = d->lm_rec.as<ekf::Dense64LmRecord>();
    const IniInView ini = view(d->ini_in, L::ini_in_layout());
    const CorrSparseView cin = view(d->corr_in, L::corr_sparse_layout(d->ld));
    LegTimer leg(elapsed_ms);
    double* pms = leg.pms();
    for (int j = 0; j < J; j++) {
        const double sx = meas_xy[2 * j], sy = meas_xy[2 * j + 1];
        const int k = *known;
        SpsView v{};
        if (k > 0) v = view(d->sps.p, L::sps_layout(k, 2, 5, true, false), false);   // (k <= n_max: inside the buffer)
        HIPC(hipEventRecord(d->e0, d->stream));
        d->finish_leave();   // (a region that is being left ends here)
        if (k > 0) {
            ekf::launch_dense64_lm_terms(d->x, d->x, sx, sy, 0, k, 0, p.r_meas, v.cols, v.Hc, v.R, v.nu, d->stream);
            score_sparse_launch(d, v, k, 2, 5, true, true, true);
        }
        ekf::launch_dense64_lm_decide(v.nis, k, k, n_max, p.gate_new, p.gate_update, p.sigma0_landmark, d->x, sx, sy, drec,
                                      ini.W, ini.xb, d->stream);
        ekf::Dense64LmRecord rec{};
        EKFC(leg(finish_timed(d, pms, {{&rec, drec, sizeof(rec)}})));
        if (best_out) best_out[j] = rec.best;
        if (rec.kind == 0) {   // dropped: nothing at all is written
            if (assoc_out) assoc_out[j] = -1;
            continue;
        }
        const bool fresh_lm = (rec.kind & ekf::kDense64LmNew) != 0, corrects = (rec.kind & ekf::kDense64LmCorrect) != 0;
        if (fresh_lm && 3 + 2 * (k + 1) > d->live) {
            if (!(flags & EKF_DENSE64_LM_GROW_LIVE))
                return fail(EKF_ERR_INVALID, fn + ": a new landmark does not fit the live dimension (grow it with "
                                                  "ekf_dense64_set_live, or pass EKF_DENSE64_LM_GROW_LIVE)");
            EKFC(ekf_dense64_set_live(d, 3 + 2 * (k + 1)));
        }
        HIPC(hipEventRecord(d->e0, d->stream));
        if (fresh_lm) init_block_launch(d, 3 + 2 * k, 2, 0, ini.W, ini.xb);   // s = 0, W = sigma0 I, xb
        if (!corrects) {   // (a gate_update <= 0: the landmark is initialised and not corrected)
            EKFC(leg(finish_timed(d, pms)));
            *known = k + 1;
            if (assoc_out) assoc_out[j] = -1;
            continue;
        }
        // the winner's operands from the current state, that is after an initialisation; the innovation wrapped (:183)
        ekf::launch_dense64_lm_terms(d->x, d->x, sx, sy, rec.win, 1, 1, p.r_meas, cin.cols, cin.Hc, cin.R, cin.nu,
                                     d->stream);
        correct_sparse_launch(d, deferred, 2, 5, true, lm_joseph(flags));
        ekf::launch_dense64_lm_wrap(d->x, view(d->corr_out, L::corr_out_layout()).verdict, d->stream);   // :187 / :385
        if (assoc_out) assoc_out[j] = -1;
        // (a refused correction's launches ran and were timed)
        const ekf_status st = leg(correct_sparse_finish(d, fnc, deferred, 2, nullptr, pms));
        if (fresh_lm && (st == EKF_OK || st == EKF_ERR_STATE)) *known = k + 1;   // the initialisation stands
        if (st != EKF_OK) return st;
        if (assoc_out) assoc_out[j] = rec.win;
    }
    return EKF_OK;
}

// ---- the same for a whole scan at once (ekf_dense64_joint.hip), shared by ekf_dense64_score_readings,
// ekf_dense64_associate_joint and ekf_dense64_associate_scan_joint ----------------------------------------------------------
constexpr int kJointReadings = ekf::kDense64JointMaxReadings, kJointPairs = ekf::kDense64JointMaxPairs;
constexpr int kJointInit = ekf::kDense64JointInitGroup;

// readings of one scoring launch against `count` landmarks: a launch stays within the sparse scoring call's rows (m = 2)
int joint_chunk(int J, int count) { return std::min(J, (kSparseRows / 2) / count); }

ekf_status joint_reserve(ekf_dense64_s* d, const char* fnc) {
    return d->joint.reserve(d->mem, L::joint_layout().bytes, true, fnc, "the joint association's buffer");
}

// J readings (in jv.xy) against landmarks [first_lm, first_lm + count), cut into launches of `chunk` readings: per launch
// [terms | score], then what the caller does with that launch's scores (first reading, readings, the view) behind it
template <class Each>
void score_readings_launch(ekf_dense64_s* d, const ekf::Params& p, const JointView& jv, int J, int first_lm, int count,
                           int chunk, bool want_nis, Each&& each) {
    const SpsView v = view(d->sps.p, L::sps_layout(chunk * count, 2, 5, true, false), false);
    for (int j0 = 0; j0 < J; j0 += chunk) {
        const int nr = std::min(chunk, J - j0);
        ekf::launch_dense64_joint_terms(d->x, d->x, jv.xy + 2 * j0, nr, first_lm, count, p.r_meas, v.cols, v.Hc, v.R, v.nu,
                                        d->stream);
        score_sparse_launch(d, v, nr * count, 2, 5, true, true, want_nis);
        each(j0, nr, v);
    }
}

// One stacked correction on pairs whose landmarks and readings sit in device memory (lm, rj: nullable = reading v): the
// operands from the current state into correct_sparse's buffer, the correction, the heading; behind e0
void joint_correct_launch(ekf_dense64_s* d, const ekf::Params& p, const JointView& jv, const int* lm, const int* rj, int V,
                          bool deferred) {
    const CorrSparseView cin = view(d->corr_in, L::corr_sparse_layout(d->ld));
    ekf::launch_dense64_joint_operands(d->x, jv.xy, lm, rj, V, p.r_meas, cin.cols, cin.Hc, cin.R, cin.nu, d->stream);
    correct_sparse_launch(d, deferred, 2 * V, 3 + 2 * V, true);
    ekf::launch_dense64_lm_wrap(d->x, view(d->corr_out, L::corr_out_layout()).verdict, d->stream);   // :187 / :385
}

// Steps 4 LIVE, 5 INIT and 6 CORRECT of THE JOINT RULE (include/ekfslam.h) on a decision that is made: rec [J] the final
// records (kind, win) on the host, n_new and n_pairs their counts, and on the device what k_djt_resolve leaves (jv.xb,
// pair_lm, pair_j, W_full, W_last).  queue_resolve runs behind this leg's e0 and in front of its first launch: nothing for
// a caller whose resolve launch is behind it already.  The live dimension once; [init per 32 new landmarks | per 30 pairs:
// operands | correction | heading wrap] with each correction's own synchronisation.
template <class Queue>
ekf_status joint_apply(ekf_dense64_s* d, const char* fnc, const ekf::Params& p, const JointView& jv, int k,
                       const ekf::Dense64LmRecord* rec, int n_new, int n_pairs, int* known, unsigned flags, int* assoc_out,
                       int* n_groups_out, LegTimer& leg, Queue&& queue_resolve) {
    const std::string fn = fnc;
    const bool deferred = (flags & EKF_DENSE64_LM_DEFERRED) != 0;
    double* pms = leg.pms();
    const int n_groups = (n_pairs + kJointPairs - 1) / kJointPairs;
    if (n_groups_out) *n_groups_out = n_groups;
    if (n_new == 0 && n_pairs == 0) return EKF_OK;   // every reading dropped: nothing at all is written
    if (3 + 2 * (k + n_new) > d->live) {
        if (!(flags & EKF_DENSE64_LM_GROW_LIVE))
            return fail(EKF_ERR_INVALID, fn + ": the new landmarks do not fit the live dimension (grow it with "
                                              "ekf_dense64_set_live, or pass EKF_DENSE64_LM_GROW_LIVE)");
        EKFC(ekf_dense64_set_live(d, 3 + 2 * (k + n_new)));
    }
    HIPC(hipEventRecord(d->e0, d->stream));
    EKFC(queue_resolve());
    for (int g0 = 0; g0 < n_new; g0 += kJointInit) {   // s = 0, W = sigma0 I, the group's xb
        const int n = std::min(kJointInit, n_new - g0);
        init_block_launch(d, 3 + 2 * (k + g0), 2 * n, 0, n == kJointInit ? jv.W_full : jv.W_last, jv.xb + 2 * g0);
    }
    if (n_pairs == 0) {   // (a gate_update <= 0: the landmarks are initialised and not corrected)
        EKFC(leg(finish_timed(d, pms)));
        *known = k + n_new;
        return EKF_OK;
    }
    int j_next = 0;   // the readings of the pairs, in ascending j, as the groups consume them
    for (int g = 0; g < n_groups; g++) {
        const int V = std::min(kJointPairs, n_pairs - g * kJointPairs);
        if (g > 0) HIPC(hipEventRecord(d->e0, d->stream));
        joint_correct_launch(d, p, jv, jv.pair_lm + g * kJointPairs, jv.pair_j + g * kJointPairs, V, deferred);
        // (a refused correction's launches ran and were timed)
        const ekf_status st = leg(correct_sparse_finish(d, fnc, deferred, 2 * V, nullptr, pms));
        if (g == 0 && (st == EKF_OK || st == EKF_ERR_STATE)) *known = k + n_new;   // the initialisations stand
        for (int v = 0; v < V; j_next++) {
            if (!(rec[j_next].kind & ekf::kDense64LmCorrect)) continue;
            if (assoc_out) assoc_out[j_next] = st == EKF_OK ? rec[j_next].win : -1;
            v++;
        }
        if (st != EKF_OK) return st;
    }
    return EKF_OK;
}

// The joint rule on J readings (include/ekfslam.h).  [upload | per launch: terms | score | argmin | resolve] and the record
// back (the FIRST synchronisation); then joint_apply.  *elapsed_ms as in associate_readings.
ekf_status associate_joint(ekf_dense64_s* d, const char* fnc, const ekf::Params& p, int J, const double* meas_xy, int n_max,
                           int* known, unsigned flags, int* assoc_out, double* best_out, int* n_groups_out,
                           double* elapsed_ms) {
    const std::string fn = fnc;
    const L::JointLayout jl = L::joint_layout();
    const JointView jv = view(d->joint.p, jl);
    LegTimer leg(elapsed_ms);
    const int k = *known;
    HIPC(hipMemcpyAsync(jv.xy, meas_xy, sizeof(double) * 2 * J, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->finish_leave();   // (a region that is being left ends here)
    if (k > 0)
        // (cut as for the full map, whatever is known: the launches stay inside the buffer reserved for it)
        score_readings_launch(d, p, jv, J, 0, k, joint_chunk(J, n_max), true, [&](int j0, int nr, const SpsView& v) {
            ekf::launch_dense64_joint_argmin(v.nis, nr, k, p.gate_new, p.gate_update, jv.pre + j0, d->stream);
        });
    else
        ekf::launch_dense64_joint_argmin(nullptr, J, 0, p.gate_new, p.gate_update, jv.pre, d->stream);
    ekf::launch_dense64_joint_resolve(jv.pre, J, k, n_max, p.gate_update, p.sigma0_landmark, d->x, jv.xy, jv.head, jv.rec,
                                      jv.pair_lm, jv.pair_j, jv.xb, jv.W_full, jv.W_last, d->stream);
    struct { int n_match, n_new, n_pairs, zero; ekf::Dense64LmRecord rec[kJointReadings]; double xb[2 * kJointReadings]; } down;
    static_assert(sizeof(down) == sizeof(int) * 4 + 32 * kJointReadings + 16 * kJointReadings, "the record of one copy");
    EKFC(leg(finish_timed(d, leg.pms(), {{&down, jv.head, jl.record_bytes}})));
    const int n_new = down.n_new, n_pairs = down.n_pairs;
    if (n_new < 0 || k + n_new > n_max || n_pairs < 0 || n_pairs > J || down.n_match < 0 || down.n_match + n_new > J)
        return fail(EKF_ERR_HIP, fn + ": the resolve kernel left an impossible record");
    for (int j = 0; j < J; j++) {
        if (best_out) best_out[j] = down.rec[j].best;
        if (assoc_out) assoc_out[j] = (down.rec[j].kind & ekf::kDense64LmCorrect) ? -2 : -1;
    }
    return joint_apply(d, fnc, p, jv, k, down.rec, n_new, n_pairs, known, flags, assoc_out, n_groups_out, leg,
                       [] { return EKF_OK; });
}

// what the joint path needs in memory: the buffer of its own, the pending panels, the scoring buffer once for the full map
ekf_status associate_joint_reserve(ekf_dense64_s* d, const char* fnc, int J, int n_max, bool deferred) {
    EKFC(joint_reserve(d, fnc));
    if (deferred) EKFC(pend_reserve(d, fnc));
    if (n_max > 0) EKFC(sps_reserve(d, L::sps_layout(joint_chunk(J, n_max) * n_max, 2, 5, true, false).bytes, fnc));
    return EKF_OK;
}

// ---- joint compatibility (ekf_dense64_jcbb.hip, ekf_dense64_jcbb.hpp), shared by ekf_dense64_jcbb_candidates,
// ekf_dense64_associate_jcbb and ekf_dense64_associate_scan_jcbb ------------------------------------------------------------
constexpr int kJcbbReadings = ekf::kDense64JcbbMaxReadings, kJcbbCand = ekf::kDense64JcbbMaxCand;
constexpr int kJcbbP = kJcbbReadings * kJcbbCand;
static_assert(kJcbbReadings == EKF_DENSE64_JCBB_MAX_READINGS && kJcbbCand == EKF_DENSE64_JCBB_MAX_CAND &&
                  kJcbbReadings == ekf::kJcbbMaxReadings && kJcbbCand == ekf::kJcbbMaxCand &&
                  ekf::kJcbbMaxNodes == EKF_DENSE64_JCBB_MAX_NODES,
              "ekfslam.h, ekf_dense64_layout.hpp and ekf_dense64_jcbb.hpp");

// what comes down in one copy (JcbbLayout from head to cols)
struct JcbbDown {
    int head[4], cand_count[kJcbbReadings], offset[kJcbbReadings], is_new[kJcbbReadings], cand_lm[kJcbbP], reading_of[kJcbbP],
        lm_of[kJcbbP];
    double best[kJcbbReadings], cand_nis[kJcbbP], nu[2 * kJcbbP];
};
static_assert(sizeof(JcbbDown) == 5264, "the record of one copy: JcbbLayout::record_bytes");

ekf_status jcbb_reserve(ekf_dense64_s* d, const char* fnc) {
    const L::JcbbLayout l = L::jcbb_layout();
    if (l.record_bytes != sizeof(JcbbDown)) return fail(EKF_ERR_HIP, std::string(fnc) + ": JcbbLayout and JcbbDown disagree");
    EKFC(d->jcbb.reserve(d->mem, l.bytes, true, fnc, "the joint compatibility buffer"));
    const size_t n = (l.bytes - l.W) / sizeof(double);   // the host's copy of W, behind the device buffer: 512 KB once
    if (d->jcbb_W.size() < n) {
        try {
            d->jcbb_W.assign(n, 0.0);
        } catch (const std::bad_alloc&) {
            return fail(EKF_ERR_NOMEM, std::string(fnc) + ": out of host memory for the cross blocks");
        }
    }
    return EKF_OK;
}

// gate_ic, the joint gates (nullable) and the node budget: the checks the jcbb calls make behind their own
ekf_status jcbb_gates_ok(const std::string& fn, const ekf::Params& p, int J, double gate_ic, const double* gate_joint,
                         long long max_nodes) {
    if (!(std::isfinite(gate_ic) && gate_ic > 0.0 && gate_ic <= p.gate_new))
        return fail(EKF_ERR_INVALID, fn + ": gate_ic must be finite and lie in (0, gate_new]");
    for (int k = 0; gate_joint && k < J; k++)
        if (!(std::isfinite(gate_joint[k]) && gate_joint[k] > 0.0))
            return fail(EKF_ERR_INVALID, fn + ": every joint gate must be finite and > 0");
    if (max_nodes < 1 || max_nodes > EKF_DENSE64_JCBB_MAX_NODES)
        return fail(EKF_ERR_INVALID, fn + ": max_nodes must lie in [1, 2^22]");
    return EKF_OK;
}

// The device half on J readings that sit in jv.xy, behind e0: the pending rows applied, [per launch: terms | score | select]
// against landmarks 0 .. k - 1 cut into launches of `chunk` readings, then [terms of the candidates | cross blocks]; the
// record and (want_W) the blocks come down behind ONE synchronisation, and the record is checked.
ekf_status jcbb_device(ekf_dense64_s* d, const char* fnc, const ekf::Params& p, const JointView& jv, int J, int k, int chunk,
                       double gate_ic, int max_cand, bool want_W, JcbbDown* down, double* elapsed_ms) {
    const L::JcbbLayout ql = L::jcbb_layout();
    const JcbbView q = view(d->jcbb.p, ql);
    const int p_cap = std::min(J * max_cand, kJcbbP);
    d->flush_pending();   // the scores, the selection and W see one Sigma in memory (a region that is being left ends here)
    auto select = [&](const double* nis, int j0, int nr) {
        ekf::launch_dense64_jcbb_select(nis, nr, k, j0, max_cand, gate_ic, p.gate_new, q.cand_count, q.cand_lm, q.cand_nis,
                                        q.best, q.is_new, d->stream);
    };
    if (k > 0)
        score_readings_launch(d, p, jv, J, 0, k, chunk, true, [&](int j0, int nr, const SpsView& v) { select(v.nis, j0, nr); });
    else
        select(nullptr, 0, J);
    ekf::launch_dense64_jcbb_terms(d->x, jv.xy, J, q.cand_count, q.cand_lm, q.head, q.offset, q.reading_of, q.lm_of, q.cols,
                                   q.Hc, q.nu, d->stream);
    if (k > 0)   // (nothing known: no candidate, P = 0, no block)
        ekf::launch_dense64_jcbb_cross(d->S, d->ld, q.head, q.cols, q.Hc, p.r_meas, p_cap, q.W, d->stream);
    // W sits at stride P, which the host does not know yet: the copy takes the 4 p_cap^2 doubles the call could fill (32 KB at
    // J = 8, 512 KB at J = 32), all inside the buffer cut for P = 128; what lies beyond 4 P^2 is never read
    EKFC(finish_timed(d, elapsed_ms, {{down, q.head, ql.record_bytes},
                                      {want_W && k > 0 ? d->jcbb_W.data() : nullptr, q.W, sizeof(double) * 4 * p_cap * p_cap}}));
    const int P = down->head[0];
    bool ok = P >= 0 && P <= p_cap;
    int sum = 0;
    for (int j = 0; j < J && ok; j++) {
        const int n = down->cand_count[j];
        ok = n >= 0 && n <= max_cand && down->offset[j] == sum;
        for (int c = 0; c < n && ok; c++) {
            const int i = down->cand_lm[j * kJcbbCand + c];
            ok = i >= 0 && i < k && sum + c < P && down->reading_of[sum + c] == j && down->lm_of[sum + c] == i;
        }
        sum += n;
    }
    if (!ok || sum != P) return fail(EKF_ERR_HIP, std::string(fnc) + ": the selection kernels left an impossible record");
    return EKF_OK;
}

// W [P][P][2][2] as it came down -> out [2P][2P] row-major in candidate order
void jcbb_unpack_W(const double* blocks, int P, double* out) {
    const size_t n = 2 * (size_t)P;
    for (int pp = 0; pp < P; pp++)
        for (int qq = 0; qq < P; qq++)
            for (int e = 0; e < 4; e++)
                out[(2 * (size_t)pp + e / 2) * n + 2 * qq + e % 2] = blocks[((size_t)pp * P + qq) * 4 + e];
}

// The whole rule on J readings (include/ekfslam.h): the device half and its one synchronisation, the search, the records
// k_djt_resolve turns into slots, positions and the pair list, then steps 4 - 6 of THE JOINT RULE through joint_apply.
ekf_status associate_jcbb(ekf_dense64_s* d, const char* fnc, const ekf::Params& p, int J, const double* meas_xy, int n_max,
                          int* known, double gate_ic, const double* gate_joint, long long max_nodes, unsigned flags,
                          int* assoc_out, double* best_out, ekf_dense64_jcbb_report* report, int* n_groups_out,
                          double* elapsed_ms) {
    const JointView jv = view(d->joint.p, L::joint_layout());
    LegTimer leg(elapsed_ms);
    const int k = *known;
    HIPC(hipMemcpyAsync(jv.xy, meas_xy, sizeof(double) * 2 * J, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    JcbbDown down;
    // (cut as for the full map, whatever is known: the launches stay inside the buffer reserved for it)
    EKFC(leg(jcbb_device(d, fnc, p, jv, J, k, n_max > 0 ? joint_chunk(J, n_max) : J, gate_ic, kJcbbCand, true, &down,
                         leg.pms())));
    const int P = down.head[0];
    std::vector<double> W(4 * (size_t)P * P);
    jcbb_unpack_W(d->jcbb_W.data(), P, W.data());
    double gates[kJcbbReadings];
    for (int m = 0; m < J; m++) gates[m] = gate_joint ? gate_joint[m] : (double)(m + 1) * gate_ic;
    int assign[kJcbbReadings];
    ekf::JcbbSearch search(J, P, down.reading_of, down.lm_of, W.data(), down.nu, gates, max_nodes);
    const ekf::JcbbResult res = search.run(assign);
    // the records: what k_djt_argmin would have left (pre), and what k_djt_resolve makes of them (fin) -- no conflicts, the
    // NEW readings in ascending j while slot < n_max
    ekf::Dense64LmRecord pre[kJcbbReadings], fin[kJcbbReadings];
    int n_new = 0, n_pairs = 0, rank = 0;
    for (int j = 0; j < J; j++) {
        ekf::Dense64LmRecord r{-1, 0, down.best[j], 0.0, 0, 0};
        if (assign[j] >= 0) r.win = down.lm_of[assign[j]], r.kind = ekf::kDense64LmCorrect;
        else if (down.is_new[j]) r.win = k, r.kind = ekf::kDense64LmNew;
        pre[j] = fin[j] = r;
        if (r.kind == ekf::kDense64LmNew) {
            fin[j].win = k + rank++;
            if (fin[j].win >= n_max) fin[j].win = -1, fin[j].kind = 0;
            else if (0.0 < p.gate_update) fin[j].kind |= ekf::kDense64LmCorrect;
        }
        n_new += (fin[j].kind & ekf::kDense64LmNew) != 0;
        n_pairs += (fin[j].kind & ekf::kDense64LmCorrect) != 0;
        if (best_out) best_out[j] = down.best[j];
        if (assoc_out) assoc_out[j] = (fin[j].kind & ekf::kDense64LmCorrect) ? -2 : -1;
    }
    if (report) *report = ekf_dense64_jcbb_report{P, res.n_pairs, n_new, J - res.n_pairs - n_new, res.exhausted, res.nodes, res.d2};
    return joint_apply(d, fnc, p, jv, k, fin, n_new, n_pairs, known, flags, assoc_out, n_groups_out, leg, [&]() -> ekf_status {
        HIPC(hipMemcpyAsync(jv.pre, pre, sizeof(ekf::Dense64LmRecord) * J, hipMemcpyHostToDevice, d->stream));
        ekf::launch_dense64_joint_resolve(jv.pre, J, k, n_max, p.gate_update, p.sigma0_landmark, d->x, jv.xy, jv.head, jv.rec,
                                          jv.pair_lm, jv.pair_j, jv.xb, jv.W_full, jv.W_last, d->stream);
        return EKF_OK;
    });
}

ekf_status associate_jcbb_reserve(ekf_dense64_s* d, const char* fnc, int J, int n_max, bool deferred) {
    EKFC(associate_joint_reserve(d, fnc, J, n_max, deferred));
    return jcbb_reserve(d, fnc);
}

// ---- the six association entry points: a rule, and the readings form or the scan form of it ------------------------------
// What tells the three rules apart in front of their run.  The jcbb members are the caller's arguments, unused by the others.
enum class Rule { kSequential, kJoint, kJcbb };
constexpr unsigned kLmFlags = EKF_DENSE64_LM_DEFERRED | EKF_DENSE64_LM_GROW_LIVE;
struct AssocRule {
    Rule rule;
    int max_readings;    // the most readings a call takes (the scan form: at most a scan's circles)
    unsigned allowed;    // the flag bits the call knows
    bool n_max_capped;   // n_max <= 32768: a scoring launch holds every landmark against one reading
    double gate_ic = 0.0;
    const double* gate_joint = nullptr;
    long long max_nodes = 0;
    ekf_dense64_jcbb_report* report = nullptr;
};
static_assert(kJointReadings == kScanClusters && kJointReadings == 128 && kJcbbReadings == 32, "the texts of the range checks");

// the argument checks in their documented order, behind the call's own (null pointers, the range of J or of the scan);
// J: the readings the call may come to have
ekf_status assoc_checks(ekf_dense64_s* d, const std::string& fn, const AssocRule& r, const ekf::Params& p, int J, int n_max,
                        const int* known, unsigned flags) {
    if (n_max < 0 || 3 + 2 * (long long)n_max > d->N)
        return fail(EKF_ERR_INVALID, fn + ": n_max must lie in [0, (N - 3) / 2]");
    if (*known < 0 || *known > n_max) return fail(EKF_ERR_INVALID, fn + ": *known must lie in [0, n_max]");
    if (3 + 2 * *known > d->live)
        return fail(EKF_ERR_INVALID, fn + ": the known landmarks must lie inside the live dimension");
    EKFC(lm_flags_ok(fn, flags, r.allowed));
    if (r.n_max_capped && n_max > kSparseRows / 2) return fail(EKF_ERR_INVALID, fn + ": n_max must not exceed 32768");
    if (r.rule == Rule::kJcbb) EKFC(jcbb_gates_ok(fn, p, J, r.gate_ic, r.gate_joint, r.max_nodes));
    return EKF_OK;
}

// what the rule needs in memory for up to J readings
ekf_status assoc_reserve(ekf_dense64_s* d, const char* fnc, const AssocRule& r, int J, int n_max, bool deferred) {
    switch (r.rule) {
        case Rule::kSequential: return associate_reserve(d, fnc, n_max, deferred);
        case Rule::kJoint: return associate_joint_reserve(d, fnc, J, n_max, deferred);
        default: return associate_jcbb_reserve(d, fnc, J, n_max, deferred);
    }
}

// the rule on J readings; *elapsed_ms (nullable) holds the time of what ran before
ekf_status assoc_run(ekf_dense64_s* d, const char* fnc, const AssocRule& r, const ekf::Params& p, int J, const double* xy,
                     int n_max, int* known, unsigned flags, int* assoc_out, double* best_out, int* n_groups_out,
                     double* elapsed_ms) {
    switch (r.rule) {
        case Rule::kSequential:
            return associate_readings(d, fnc, p, J, xy, n_max, known, flags, assoc_out, best_out, elapsed_ms);
        case Rule::kJoint:
            return associate_joint(d, fnc, p, J, xy, n_max, known, flags, assoc_out, best_out, n_groups_out, elapsed_ms);
        default:
            return associate_jcbb(d, fnc, p, J, xy, n_max, known, r.gate_ic, r.gate_joint, r.max_nodes, flags, assoc_out,
                                  best_out, r.report, n_groups_out, elapsed_ms);
    }
}

// Both forms between their own checks and their first launch: the remaining checks, behind the last of them the presets of
// every output (a refused call has written to none), the device, the memory for `cap` readings.
ekf_status assoc_begin(ekf_dense64_s* d, const char* fnc, const AssocRule& r, const ekf::Params& p, int cap, int n_max,
                       const int* known, unsigned flags, int* count_out, double* centres_out, int* assoc_out,
                       double* best_out, int* n_groups_out, double* elapsed_ms) {
    EKFC(assoc_checks(d, fnc, r, p, cap, n_max, known, flags));
    if (elapsed_ms) *elapsed_ms = 0.0;
    if (count_out) *count_out = 0;
    if (n_groups_out) *n_groups_out = 0;
    if (r.report) *r.report = ekf_dense64_jcbb_report{0, 0, 0, 0, 0, 0, 0.0};
    for (int j = 0; j < cap; j++) {
        if (assoc_out) assoc_out[j] = -2;
        if (best_out) best_out[j] = p.gate_new;
        if (centres_out) centres_out[2 * j] = centres_out[2 * j + 1] = 0.0;
    }
    HIPC(hipSetDevice(d->device));
    return assoc_reserve(d, fnc, r, cap, n_max, (flags & EKF_DENSE64_LM_DEFERRED) != 0);
}

// The readings form: J readings from the caller.  The sequential rule without the Joseph form is inside a region's terms.
ekf_status assoc_readings_form(ekf_dense64_s* d, const char* fnc, const AssocRule& r, const ekf_params* params, int J,
                               const double* meas_xy, int n_max, int* known, unsigned flags, int* assoc_out,
                               double* best_out, int* n_groups_out, double* elapsed_ms) {
    const std::string fn = fnc;
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    const bool in_terms = r.rule == Rule::kSequential && !(flags & EKF_DENSE64_LM_JOSEPH);
    const RegionLeave leaving(in_terms ? nullptr : d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!known || !meas_xy) return fail(EKF_ERR_INVALID, fn + ": null argument");
    if (J < 1 || J > r.max_readings)
        return fail(EKF_ERR_INVALID, fn + (r.max_readings == INT_MAX         ? ": J must be at least 1"
                                           : r.max_readings == kJcbbReadings ? ": J must lie in [1, 32]"
                                                                             : ": J must lie in [1, 128]"));
    const ekf::Params p = landmark_params(params);
    EKFC(assoc_begin(d, fnc, r, p, J, n_max, known, flags, nullptr, nullptr, assoc_out, best_out, n_groups_out, elapsed_ms));
    return assoc_run(d, fnc, r, p, J, meas_xy, n_max, known, flags, assoc_out, best_out, n_groups_out, elapsed_ms);
}

// The scan form: ekf_dense64_fit_scan, then the rule on the first min(count, max_readings) centres.  Checked and reserved
// for max_readings, whatever the scan turns out to hold; the fit's time is the first leg of *elapsed_ms.
ekf_status assoc_scan_form(ekf_dense64_s* d, const char* fnc, const AssocRule& r, const ekf_params* params,
                           const double* ranges, int n_beams, int max_readings, int n_max, int* known, unsigned flags,
                           int* count_out, double* centres_out, int* assoc_out, double* best_out, double* elapsed_ms) {
    const std::string fn = fnc;
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!ranges || !count_out || !known) return fail(EKF_ERR_INVALID, fn + ": null argument");
    const int most = std::min(r.max_readings, kScanClusters);
    if (n_beams < 1 || n_beams > kScanBeams || max_readings < 1 || max_readings > most)
        return fail(EKF_ERR_INVALID, fn + (most == kJcbbReadings ? ": n_beams must lie in [1, 1024] and max_readings in [1, 32]"
                                                                 : ": n_beams must lie in [1, 1024] and max_readings in [1, 128]"));
    const ekf::Params p = landmark_params(params);
    EKFC(assoc_begin(d, fnc, r, p, max_readings, n_max, known, flags, count_out, centres_out, assoc_out, best_out, nullptr,
                     elapsed_ms));
    ScanRecord rec{};
    EKFC(scan_fit(d, fnc, ranges, n_beams, max_readings, false, elapsed_ms, &rec));
    const int J = rec.count;   // (the kernel keeps the first max_readings circles in cluster order)
    *count_out = J;
    if (J == 0) return EKF_OK;
    double xy[2 * kScanClusters];   // the rule's launches leave d->scan_rec alone; a copy keeps that out of the argument
    std::memcpy(xy, rec.centres, sizeof(double) * 2 * J);
    if (centres_out) std::memcpy(centres_out, xy, sizeof(double) * 2 * J);
    return assoc_run(d, fnc, r, p, J, xy, n_max, known, flags, assoc_out, best_out, nullptr, elapsed_ms);
}

}  // namespace

extern "C" {

ekf_status ekf_dense64_set_state(ekf_dense64_handle d, const double* x) {
    if (!d || !x) return fail(EKF_ERR_INVALID, "ekf_dense64_set_state: null argument");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    HIPC(hipSetDevice(d->device));
    d->finish_leave();   // (a region that is being left ends here)
    HIPC(hipMemcpyAsync(d->x, x, sizeof(double) * d->N, hipMemcpyHostToDevice, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}
ekf_status ekf_dense64_get_state(ekf_dense64_handle d, double* out) {
    if (!d || !out) return fail(EKF_ERR_INVALID, "ekf_dense64_get_state: null argument");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    HIPC(hipSetDevice(d->device));
    d->finish_leave();   // (a region that is being left ends here)
    HIPC(hipMemcpyAsync(out, d->x, sizeof(double) * d->N, hipMemcpyDeviceToHost, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}
ekf_status ekf_dense64_get_state_block(ekf_dense64_handle d, int first, int count, double* out) {
    return dense64_state_block("ekf_dense64_get_state_block", d, first, count, out, nullptr);
}
ekf_status ekf_dense64_set_state_block(ekf_dense64_handle d, int first, int count, const double* x) {
    return dense64_state_block("ekf_dense64_set_state_block", d, first, count, nullptr, x);
}

// One correction: the operands go up (H twice: as given, zero padded to ld, and transposed with m rounded up to 16), the six
// launches are timed by the handle's events, the verdict and nis come back in one copy.
ekf_status ekf_dense64_correct(ekf_dense64_handle d, int m, const double* H, const double* R, const double* nu,
                               double* nis_out, double* elapsed_ms) {
    if (!d || !H || !R || m < 1 || m > kMaxM || m > d->N || (nis_out && !nu))
        return fail(EKF_ERR_INVALID, "ekf_dense64_correct: bad argument");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    HIPC(hipSetDevice(d->device));
    const int N = d->N, ld = d->ld;
    const L::CorrInLayout l = L::corr_in_layout(ld);
    const int mp = round_up(m, 16);   // row length of the transposed copy
    d->host_in.assign(l.bytes / sizeof(double), 0.0);
    const CorrInView h = view(d->host_in.data(), l), in = view(d->corr_in, l);
    for (int k = 0; k < m; k++)
        for (int j = 0; j < N; j++) {
            const double v = H[(size_t)k * N + j];
            h.H[(size_t)k * ld + j] = v;
            h.Ht[(size_t)j * mp + k] = v;
        }
    std::memcpy(h.R, R, sizeof(double) * m * m);
    if (nu) std::memcpy(h.nu, nu, sizeof(double) * m);
    HIPC(hipMemcpyAsync(in.H, h.H, sizeof(double) * m * ld, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(in.Ht, h.Ht, sizeof(double) * ld * mp, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(in.R, h.R, l.bytes - l.R, hipMemcpyHostToDevice, d->stream));   // R and nu, adjacent
    const CorrOutView out = view(d->corr_out, L::corr_out_layout());
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    ekf::launch_dense64_correct(d->pl_full, d->S, d->x, d->workspace(), in.H, in.Ht, in.R, nu ? in.nu : nullptr, m, out.nis,
                                out.verdict, d->stream);
    double nis = 0.0;
    int verdict = 0;
    EKFC(finish_correction(d, elapsed_ms, &nis, &verdict));
    if (verdict != 0)
        return fail(EKF_ERR_STATE, "ekf_dense64_correct: H Sigma H^T + R is singular or not finite (zero or non-finite "
                                   "pivot); state and Sigma are unchanged");
    if (nis_out) *nis_out = nis;
    return EKF_OK;
}

// Scoring of J candidates.  The Jacobians go straight from the caller's array into their row groups on the device (one
// strided copy when m divides 64, one per group otherwise); the outputs come straight back into the caller's arrays.
ekf_status ekf_dense64_score(ekf_dense64_handle d, int J, int m, const double* H, const double* R, int r_shared,
                             const double* nu, double* nis_out, double* S_out, int* flag_out, double* elapsed_ms) {
    const char *fn = "ekf_dense64_score", *what = "the candidates' buffers";
    if (!d || !H || !R || J < 1 || m < 1 || m > kMaxM || m > d->N || (long long)J * m > kScoreRows ||
        (nis_out && !nu) || (!nis_out && !S_out && !flag_out))
        return fail(EKF_ERR_INVALID, "ekf_dense64_score: bad argument");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    HIPC(hipSetDevice(d->device));
    const int N = d->N, ld = d->ld;
    const ekf::Dense64ScorePlan sp = ekf::dense64_score_plan(N, ld, J, m);
    const bool own_ws = sp.spart_doubles > (size_t)ld * ld;   // else the product buffer, dead between propagations
    if (!d->sc_small.p) {
        const hipError_t e = ekf::dense64_score_prepare();
        if (e != hipSuccess) return Ledger::refuse(e, fn, what);
    }
    EKFC(d->sc_small.reserve(d->mem, L::sc_small_layout().bytes, false, fn, what));
    EKFC(d->sc_H.reserve(d->mem, sizeof(double) * sp.h_doubles, true, fn, what));
    if (own_ws) EKFC(d->sc_ws.reserve(d->mem, sizeof(double) * sp.spart_doubles, false, fn, what));
    const size_t mm = (size_t)m * m, w = sizeof(double) * N;
    const int per = sp.cpg * m;   // rows of a full group
    double* Hs = d->sc_H.as<double>();
    if (per == ekf::kDense64ScoreGroup) {
        HIPC(hipMemcpy2DAsync(Hs, sizeof(double) * ld, H, w, w, (size_t)J * m, hipMemcpyHostToDevice, d->stream));
    } else {
        for (int g = 0; g < sp.n_groups; g++) {
            const int rows = std::min(sp.cpg, J - g * sp.cpg) * m;
            HIPC(hipMemcpy2DAsync(Hs + (size_t)g * ekf::kDense64ScoreGroup * ld, sizeof(double) * ld,
                                  H + (size_t)g * per * N, w, w, rows, hipMemcpyHostToDevice, d->stream));
        }
    }
    const ScSmallView sm = view(d->sc_small.p, L::sc_small_layout());
    HIPC(hipMemcpyAsync(sm.R, R, sizeof(double) * (r_shared ? mm : J * mm), hipMemcpyHostToDevice, d->stream));
    if (nu) HIPC(hipMemcpyAsync(sm.nu, nu, sizeof(double) * J * m, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    ekf::launch_dense64_score(sp, d->S, Hs, own_ws ? d->sc_ws.as<double>() : d->T, sm.R, r_shared ? 1 : 0,
                              nu ? sm.nu : nullptr, J, m, nis_out ? sm.nis : nullptr, sm.S, sm.flag, d->stream);
    return finish_timed(d, elapsed_ms, {{nis_out, sm.nis, sizeof(double) * J},
                                        {S_out, sm.S, sizeof(double) * J * mm},
                                        {flag_out, sm.flag, sizeof(int) * J}});
}

// The block-structured prediction: Fr, Qr and dx go up, one launch, timed by the handle's events.  The pending rows go
// through the same congruence when the handle carries them (ekf_dense64_carry.hip).  The stored F and Q are not involved.
ekf_status ekf_dense64_propagate_block(ekf_dense64_handle d, int first, int r, const double* Fr, const double* Qr,
                                       const double* dx, double* elapsed_ms) {
    if (!d || !Fr || r < 1 || r > kMaxR || first < 0 || r > d->live || first > d->live - r)
        return fail(EKF_ERR_INVALID, "ekf_dense64_propagate_block: bad argument (the block must lie inside the live dimension)");
    HIPC(hipSetDevice(d->device));
    const BlkInView in = view(d->blk_in, L::blk_in_layout());
    const size_t rr = sizeof(double) * r * r;
    HIPC(hipMemcpyAsync(in.Fr, Fr, rr, hipMemcpyHostToDevice, d->stream));
    if (Qr) HIPC(hipMemcpyAsync(in.Qr, Qr, rr, hipMemcpyHostToDevice, d->stream));
    if (dx) HIPC(hipMemcpyAsync(in.dx, dx, sizeof(double) * r, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->carry_or_flush([&](const PendView& p) {
        ekf::launch_dense64_panel_map(p.K, p.T, d->pend_rows, in.Fr, nullptr, d->ld, first, r, r, d->stream);
    });
    ekf::launch_dense64_block(d->S, d->x, in.Fr, Qr ? in.Qr : nullptr, dx ? in.dx : nullptr, d->live, d->ld, first, r,
                              d->stream);
    d->region_row_map(in.Fr, nullptr, first, r, r);
    return finish_timed(d, elapsed_ms);
}

ekf_status ekf_dense64_correct_sparse(ekf_dense64_handle d, int m, int s, const int* cols, const double* Hc,
                                      const double* R, const double* nu, double* nis_out, double* elapsed_ms) {
    return dense64_correct_sparse(d, false, m, s, cols, Hc, R, nu, nis_out, elapsed_ms);
}
ekf_status ekf_dense64_correct_sparse_deferred(ekf_dense64_handle d, int m, int s, const int* cols, const double* Hc,
                                               const double* R, const double* nu, double* nis_out, double* elapsed_ms) {
    return dense64_correct_sparse(d, true, m, s, cols, Hc, R, nu, nis_out, elapsed_ms);
}

ekf_status ekf_dense64_correct_sparse_joseph(ekf_dense64_handle d, int m, int s, const int* cols, const double* Hc,
                                             const double* R, const double* nu, const double* gain_w, double* nis_out,
                                             long long* tiles_skipped, double* elapsed_ms) {
    return dense64_correct_sparse_joseph(d, m, s, cols, Hc, R, nu, gain_w, nis_out, tiles_skipped, elapsed_ms);
}
ekf_status ekf_dense64_joseph_launch_info(ekf_dense64_handle d, int* tile_rows, int* tile_cols, int* threads) {
    if (!d || !tile_rows || !tile_cols || !threads)
        return fail(EKF_ERR_INVALID, "ekf_dense64_joseph_launch_info: null argument");
    *tile_rows = ekf::kDense64JosephTileRows;
    *tile_cols = ekf::kDense64JosephTileCols;
    *threads = ekf::kDense64JosephThreads;
    return EKF_OK;
}

ekf_status ekf_dense64_flush(ekf_dense64_handle d, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_flush: null handle");
    if (elapsed_ms) *elapsed_ms = 0.0;
    if (d->pend_rows == 0) return EKF_OK;
    HIPC(hipSetDevice(d->device));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    return finish_timed(d, elapsed_ms);
}
ekf_status ekf_dense64_pending(ekf_dense64_handle d, int* rows) {
    if (!d || !rows) return fail(EKF_ERR_INVALID, "ekf_dense64_pending: null argument");
    *rows = d->pend_rows;
    return EKF_OK;
}
ekf_status ekf_dense64_set_carry(ekf_dense64_handle d, int on) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_set_carry: null handle");
    d->carry = on ? 1 : 0;
    return EKF_OK;
}
ekf_status ekf_dense64_get_carry(ekf_dense64_handle d, int* on) {
    if (!d || !on) return fail(EKF_ERR_INVALID, "ekf_dense64_get_carry: null argument");
    *on = d->carry;
    return EKF_OK;
}

ekf_status ekf_dense64_score_sparse(ekf_dense64_handle d, int J, int m, int s, const int* cols, const double* Hc,
                                    const double* R, int r_shared, const double* nu, double* nis_out, double* S_out,
                                    int* flag_out, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_score_sparse: null handle");
    if (!cols || !Hc || !R || J < 1 || m < 1 || m > kMaxM || m > d->live || s < 1 || s > kMaxS || s > d->live ||
        (long long)J * m > kSparseRows || (nis_out && !nu) || (!nis_out && !S_out && !flag_out))
        return fail(EKF_ERR_INVALID, "ekf_dense64_score_sparse: bad argument");
    if (!index_lists_ok(d->host_stamp, d->live, J, s, cols))
        return fail(EKF_ERR_INVALID, "ekf_dense64_score_sparse: every row of cols must hold distinct indices in [0, N), "
                                     "below the live dimension");
    HIPC(hipSetDevice(d->device));
    const size_t mm = (size_t)m * m;
    const L::SpsLayout l = L::sps_layout(J, m, s, r_shared != 0, S_out != nullptr);
    EKFC(sps_reserve(d, l.bytes, "ekf_dense64_score_sparse"));
    const SpsView v = view(d->sps.p, l, S_out != nullptr);
    HIPC(hipMemcpyAsync(v.Hc, Hc, sizeof(double) * J * m * s, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(v.R, R, sizeof(double) * (r_shared ? mm : J * mm), hipMemcpyHostToDevice, d->stream));
    if (nu) HIPC(hipMemcpyAsync(v.nu, nu, sizeof(double) * J * m, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(v.cols, cols, sizeof(int) * J * s, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    score_sparse_launch(d, v, J, m, s, r_shared != 0, nu != nullptr, nis_out != nullptr);
    return finish_timed(d, elapsed_ms, {{nis_out, v.nis, sizeof(double) * J},
                                        {S_out, v.S, sizeof(double) * J * mm},
                                        {flag_out, v.flag, sizeof(int) * J}});
}

// G, W, xb and the list go up into the buffer allocated with the handle, one launch, timed by the handle's events.  The
// stored F and Q of the handle are not involved.
ekf_status ekf_dense64_init_block(ekf_dense64_handle d, int first, int r, int s, const int* cols, const double* G,
                                  const double* W, const double* xb, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_init_block: null handle");
    if (r < 1 || r > kMaxR || r > d->live || first < 0 || first > d->live - r || s < 0 || s > kMaxS || s > d->live - r ||
        (s > 0 && (!cols || !G)))
        return fail(EKF_ERR_INVALID, "ekf_dense64_init_block: bad argument (the block must lie inside the live dimension)");
    if (s > 0) {
        if (!index_lists_ok(d->host_stamp, d->live, 1, s, cols))
            return fail(EKF_ERR_INVALID, "ekf_dense64_init_block: cols must hold distinct indices in [0, N), below the live "
                                         "dimension");
        for (int k = 0; k < s; k++)
            if (cols[k] >= first && cols[k] < first + r)
                return fail(EKF_ERR_INVALID, "ekf_dense64_init_block: no index of cols may lie inside [first, first + r) "
                                             "(the in-place case is ekf_dense64_propagate_block)");
    }
    HIPC(hipSetDevice(d->device));
    const IniInView in = view(d->ini_in, L::ini_in_layout());
    if (s > 0) {
        HIPC(hipMemcpyAsync(in.G, G, sizeof(double) * r * s, hipMemcpyHostToDevice, d->stream));
        HIPC(hipMemcpyAsync(in.cols, cols, sizeof(int) * s, hipMemcpyHostToDevice, d->stream));
    }
    if (W) HIPC(hipMemcpyAsync(in.W, W, sizeof(double) * r * r, hipMemcpyHostToDevice, d->stream));
    if (xb) HIPC(hipMemcpyAsync(in.xb, xb, sizeof(double) * r, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    init_block_launch(d, first, r, s, W ? in.W : nullptr, xb ? in.xb : nullptr);
    return finish_timed(d, elapsed_ms);
}

// The exchange of two blocks: nothing goes up.  The pending rows take the same permutation (a congruence with A = P) when
// the handle carries them, and are applied first otherwise.
ekf_status ekf_dense64_swap_blocks(ekf_dense64_handle d, int first_a, int first_b, int r, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_swap_blocks: null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (r < 1 || r > kMaxR || r > d->live || first_a < 0 || first_b < 0 || first_a > d->live - r || first_b > d->live - r)
        return fail(EKF_ERR_INVALID, "ekf_dense64_swap_blocks: bad argument (both blocks must lie inside the live dimension)");
    if (std::abs(first_a - first_b) < r)
        return fail(EKF_ERR_INVALID, "ekf_dense64_swap_blocks: the blocks must be disjoint, |first_a - first_b| >= r");
    HIPC(hipSetDevice(d->device));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->carry_or_flush([&](const PendView& p) {
        ekf::launch_dense64_panel_swap(p.K, p.T, d->pend_rows, d->ld, first_a, first_b, r, d->stream);
    });
    ekf::launch_dense64_swap(d->S, d->x, d->live, d->ld, first_a, first_b, r, d->stream);
    return finish_timed(d, elapsed_ms);
}

// out[a][c] = Sigma[rows[a]][cols[c]]: the two lists go up, one gather launch into the handle's buffer, one copy back.
ekf_status ekf_dense64_get_sigma_block(ekf_dense64_handle d, int nr, const int* rows, int nc, const int* cols,
                                       double* out) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_get_sigma_block: null handle");
    if (!rows || !cols || !out || nr < 1 || nc < 1 || (long long)nr * nc > kReadMax)
        return fail(EKF_ERR_INVALID, "ekf_dense64_get_sigma_block: bad argument");
    for (int a = 0; a < nr; a++)
        if (rows[a] < 0 || rows[a] >= d->N)
            return fail(EKF_ERR_INVALID, "ekf_dense64_get_sigma_block: every index of rows must lie in [0, N)");
    for (int c = 0; c < nc; c++)
        if (cols[c] < 0 || cols[c] >= d->N)
            return fail(EKF_ERR_INVALID, "ekf_dense64_get_sigma_block: every index of cols must lie in [0, N)");
    if (d->region_on)
        for (int e = 0; e < nr + nc; e++)
            if ((e < nr ? rows[e] : cols[e - nr]) >= d->live) {   // an index beyond the region: it ends first
                d->leave_region();
                break;
            }
    HIPC(hipSetDevice(d->device));
    const RdBufView rd = view(d->rd_buf, L::rd_buf_layout());
    HIPC(hipMemcpyAsync(rd.rows, rows, sizeof(int) * nr, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(rd.cols, cols, sizeof(int) * nc, hipMemcpyHostToDevice, d->stream));
    if (d->carries()) {   // Sigma_cur through the pending rows; read-only
        const PendView p = d->panels();
        ekf::launch_dense64_read_block_deferred(d->S, p.K, p.T, d->pend_rows, rd.rows, rd.cols, rd.out, nr, nc, d->ld, d->N,
                                                d->live, d->stream);
    } else {
        d->flush_pending();
        ekf::launch_dense64_read_block(d->S, rd.rows, rd.cols, rd.out, nr, nc, d->ld, d->stream);
    }
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out, rd.out, sizeof(double) * nr * nc, hipMemcpyDeviceToHost, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}

// The live dimension.  Growing: a pending row is zero on [old, ld) whatever the panels hold there from wider calls, so those
// columns of the p waiting rows of both panels are set to zero -- up to the new width rounded up to 128, what the calls of
// that width keep zero -- and nothing is flushed.  Shrinking: the rows have support up to the old width, so they are applied
// first, at the old width.
ekf_status ekf_dense64_set_live(ekf_dense64_handle d, int Na) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_set_live: null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (Na < 1 || Na > d->N) return fail(EKF_ERR_INVALID, "ekf_dense64_set_live: the live dimension must lie in [1, N]");
    d->finish_leave();   // (a region that is being left ends here)
    if (Na == d->live) return EKF_OK;
    if (d->pend_rows > 0) {
        HIPC(hipSetDevice(d->device));
        if (Na < d->live) {
            d->flush_pending();
        } else {
            const int upto = std::min(d->ld, round_up(Na, ekf::kDenseTile));
            const PendView p = d->panels();
            for (double* panel : {p.K, p.T})
                HIPC(hipMemset2DAsync(panel + d->live, sizeof(double) * d->ld, 0, sizeof(double) * (upto - d->live),
                                      d->pend_rows, d->stream));
        }
        HIPC(hipGetLastError());
        HIPC(hipStreamSynchronize(d->stream));
    }
    d->live = Na;
    d->pl_live = ekf::dense64_live_plan(d->pl_full, Na);
    return EKF_OK;
}
ekf_status ekf_dense64_get_live(ekf_dense64_handle d, int* Na) {
    if (!d || !Na) return fail(EKF_ERR_INVALID, "ekf_dense64_get_live: null argument");
    *Na = d->live;
    return EKF_OK;
}

// ---- a local region (ekf_dense64_region.hip) ------------------------------------------------------------------------------
// The accumulators and the scratch of the global update are one all-or-nothing group of the ledger, kept for the next
// region that needs no more; the pending rows are applied at the old width, live becomes Na, Phi = I, Psi = 0, theta = 0.
ekf_status ekf_dense64_region_begin(ekf_dense64_handle d, int Na, double* elapsed_ms) {
    const char* fn = "ekf_dense64_region_begin";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    if (d->region_on) return fail(EKF_ERR_STATE, std::string(fn) + ": a region is open already (ekf_dense64_region_end first)");
    if (Na < ekf::kDense64RegionMinNa || Na >= d->N)
        return fail(EKF_ERR_INVALID, std::string(fn) + ": the region must hold 3 <= Na < N states");
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64RegionPlan pl = ekf::dense64_region_plan(Na, d->N, d->ld);
    EKFC(d->region_mem.reserve(d->mem, pl, fn));   // all or nothing; on a failure nothing has changed
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();   // at the old width
    ekf::launch_dense64_region_reset(pl, d->region_mem.acc, d->stream);
    EKFC(finish_timed(d, elapsed_ms));
    d->region_pl = pl;
    d->region_back = d->live;
    d->live = Na;
    d->pl_live = ekf::dense64_live_plan(d->pl_full, Na);
    d->region_on = 1;
    d->region_corrections = d->region_row_maps = 0;
    return EKF_OK;
}

ekf_status ekf_dense64_region_end(ekf_dense64_handle d, ekf_dense64_region_report* report, double* elapsed_ms) {
    const char* fn = "ekf_dense64_region_end";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    if (!d->region_on) return fail(EKF_ERR_STATE, std::string(fn) + ": no region is open");
    HIPC(hipSetDevice(d->device));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->close_region();
    if (report)
        *report = ekf_dense64_region_report{d->region_pl.Na, d->region_pl.nb, d->region_corrections, d->region_row_maps,
                                            (long long)d->region_mem.held};
    return finish_timed(d, elapsed_ms);
}

ekf_status ekf_dense64_region_info(ekf_dense64_handle d, int* active, int* Na, long long* corrections, long long* row_maps,
                                   long long* ended_by_other_call) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_region_info: null handle");
    if (active) *active = d->region_on;
    if (Na) *Na = d->region_on ? d->region_pl.Na : 0;
    if (corrections) *corrections = d->region_corrections;
    if (row_maps) *row_maps = d->region_row_maps;
    if (ended_by_other_call) *ended_by_other_call = d->region_ended_by_other;
    return EKF_OK;
}

// Test hook: the buffers as they sit in memory, padding included (which every kernel of the handle has to keep at +0).
ekf_status ekf_dense64_get_padded(ekf_dense64_handle d, double* sigma_out, double* state_out) {
    if (!d || (!sigma_out && !state_out)) return fail(EKF_ERR_INVALID, "ekf_dense64_get_padded: null argument");
    HIPC(hipSetDevice(d->device));
    d->sigma_needed();
    HIPC(hipGetLastError());
    if (sigma_out) HIPC(hipMemcpyAsync(sigma_out, d->S, sizeof(double) * d->ld * d->ld, hipMemcpyDeviceToHost, d->stream));
    if (state_out) HIPC(hipMemcpyAsync(state_out, d->x, sizeof(double) * d->ld, hipMemcpyDeviceToHost, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}

ekf_status ekf_dense64_region_launch_info(ekf_dense64_handle d, int Na, int* tile_rows, int* tile_cols, int* threads,
                                          int* pitch, int* update_tiles, int* gemm_tiles, int* gemm_k,
                                          long long* group_bytes) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_region_launch_info: null handle");
    if (Na < ekf::kDense64RegionMinNa || Na >= d->N)
        return fail(EKF_ERR_INVALID, "ekf_dense64_region_launch_info: 3 <= Na < N");
    const ekf::Dense64RegionPlan pl = ekf::dense64_region_plan(Na, d->N, d->ld);
    if (tile_rows) *tile_rows = ekf::kDense64RegionTileRows;
    if (tile_cols) *tile_cols = ekf::kDense64RegionTileCols;
    if (threads) *threads = ekf::kDense64RegionThreads;
    if (pitch) *pitch = pl.pitch;
    if (update_tiles) *update_tiles = pl.upd_tiles_r * pl.upd_tiles_c;
    if (gemm_tiles) *gemm_tiles = pl.gemm_tiles * pl.gemm_tiles;
    if (gemm_k) *gemm_k = pl.gemm_k;
    if (group_bytes) *group_bytes = (long long)pl.group_bytes;
    return EKF_OK;
}

// One streaming launch over the two rectangles; the two result words sit where a correction's nis and verdict do.
ekf_status ekf_dense64_coupling(ekf_dense64_handle d, int Na, long long* nonzero, double* max_abs, double* elapsed_ms) {
    if (!d || !nonzero) return fail(EKF_ERR_INVALID, "ekf_dense64_coupling: null argument");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (Na < 1 || Na > d->N) return fail(EKF_ERR_INVALID, "ekf_dense64_coupling: Na must lie in [1, N]");
    HIPC(hipSetDevice(d->device));
    static_assert(sizeof(unsigned long long) == sizeof(double), "two words in corr_out");
    unsigned long long out[2] = {0, 0};
    HIPC(hipMemsetAsync(d->corr_out, 0, sizeof(out), d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    ekf::launch_dense64_coupling(d->S, d->N, d->ld, Na, view(d->corr_out, L::corr_out_layout()).words, d->stream);
    EKFC(finish_timed(d, elapsed_ms, {{out, d->corr_out, sizeof(out)}}));
    *nonzero = (long long)out[0];
    if (max_abs) std::memcpy(max_abs, &out[1], sizeof(double));
    return EKF_OK;
}

// ---- the health of the live corner and its symmetrisation (ekf_dense64_health.hip) ----------------------------------------
ekf_status ekf_dense64_health_launch_info(ekf_dense64_handle d, int* tile, int* threads) {
    if (!d || !tile || !threads) return fail(EKF_ERR_INVALID, "ekf_dense64_health_launch_info: null argument");
    *tile = ekf::kDense64HealthTile;
    *threads = ekf::kDense64HealthThreads;
    return EKF_OK;
}

namespace {
// the workspace for the live dimension and its result words set to zero; before e0
ekf_status health_reserve(ekf_dense64_s* d, const char* fn, ekf::Dense64HealthPlan* pl) {
    *pl = ekf::dense64_health_plan(d->live);
    EKFC(d->health.reserve(d->mem, pl->bytes, false, fn, "the health pass's workspace"));
    HIPC(hipMemsetAsync(d->health.as<char>() + pl->off_words, 0, sizeof(unsigned long long) * ekf::kDense64HealthWords, d->stream));
    return EKF_OK;
}
}  // namespace

// The result words are zeroed, the pending rows applied, three launches; the words come back behind the one synchronisation.
ekf_status ekf_dense64_health(ekf_dense64_handle d, ekf_dense64_health_report* out, double* elapsed_ms) {
    const char* fn = "ekf_dense64_health";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!out) return fail(EKF_ERR_INVALID, std::string(fn) + ": null report");
    HIPC(hipSetDevice(d->device));
    ekf::Dense64HealthPlan pl;
    EKFC(health_reserve(d, fn, &pl));
    unsigned long long w[ekf::kDense64HealthWords] = {};
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    ekf::launch_dense64_health(pl, d->S, d->ld, d->health.p, d->stream);
    EKFC(finish_timed(d, elapsed_ms, {{w, d->health.as<char>() + pl.off_words, sizeof(w)}}));
    const bool pair = w[ekf::kDense64HealthMaxLoc] != ~0ull;
    *out = ekf_dense64_health_report{};
    out->n_nonfinite = (long long)w[ekf::kDense64HealthNonfinite];
    out->n_asym = (long long)w[ekf::kDense64HealthAsym];
    out->n_diag_bad = (long long)w[ekf::kDense64HealthDiagBad];
    out->n_minor = (long long)w[ekf::kDense64HealthMinor];
    std::memcpy(&out->max_asym, &w[ekf::kDense64HealthMaxBits], sizeof(double));
    std::memcpy(&out->min_diag, &w[ekf::kDense64HealthMinDiag], sizeof(double));
    out->asym_i = pair ? (int)(w[ekf::kDense64HealthMaxLoc] >> 32) : -1;
    out->asym_j = pair ? (int)(w[ekf::kDense64HealthMaxLoc] & 0xffffffffull) : -1;
    out->min_diag_i = (int)(long long)w[ekf::kDense64HealthMinDiagIdx];
    return EKF_OK;
}

// The result words are zeroed, the pending rows applied, one launch in place.
ekf_status ekf_dense64_symmetrize(ekf_dense64_handle d, long long* n_changed, double* max_asym, double* elapsed_ms) {
    const char* fn = "ekf_dense64_symmetrize";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    HIPC(hipSetDevice(d->device));
    ekf::Dense64HealthPlan pl;
    EKFC(health_reserve(d, fn, &pl));
    unsigned long long w[ekf::kDense64HealthWords] = {};
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    ekf::launch_dense64_symmetrize(pl, d->S, d->ld, d->health.p, d->stream);
    EKFC(finish_timed(d, elapsed_ms, {{w, d->health.as<char>() + pl.off_words, sizeof(w)}}));
    if (n_changed) *n_changed = (long long)w[ekf::kDense64HealthAsym];
    if (max_asym) std::memcpy(max_asym, &w[ekf::kDense64HealthMaxBits], sizeof(double));
    return EKF_OK;
}

// ---- what observing each landmark would gain (ekf_dense64_value.hip) --------------------------------------------------------
ekf_status ekf_dense64_value_launch_info(ekf_dense64_handle d, int* tile_rows, int* tile_lm, int* threads) {
    if (!d || !tile_rows || !tile_lm || !threads) return fail(EKF_ERR_INVALID, "ekf_dense64_value_launch_info: null argument");
    *tile_rows = ekf::kDense64ValueTileRows;
    *tile_lm = ekf::kDense64ValueTileLm;
    *threads = ekf::kDense64ValueThreads;
    return EKF_OK;
}

namespace {
static_assert(sizeof(ekf_dense64_value_best) == sizeof(ekf::Dense64ValueBest), "ekfslam.h and ekf_dense.hpp");

struct ValueOut {
    double *dtrace, *dtrace_pose, *detS, *S;
    int* flag;
    ekf_dense64_value_best* best;
    bool none() const { return !dtrace && !dtrace_pose && !detS && !S && !flag && !best; }
};

// The checks both calls share, in the documented order behind the NULL handle; the caller holds the RegionLeave.
ekf_status value_checks(ekf_dense64_s* d, const std::string& fn, int first_lm, int count, bool any_out) {
    if (!any_out) return fail(EKF_ERR_INVALID, fn + ": every output is NULL");
    if (count < 1 || first_lm < 0) return fail(EKF_ERR_INVALID, fn + ": count >= 1 and first_lm >= 0");
    if (3 + 2 * ((long long)first_lm + count) > d->live)
        return fail(EKF_ERR_INVALID, fn + ": the landmarks must lie inside the live dimension");
    return EKF_OK;
}

// The pending rows applied, four launches on operands that sit in the workspace, everything asked for back behind the one
// synchronisation; behind e0.
ekf_status value_run(ekf_dense64_s* d, const ekf::Dense64ValuePlan& pl, const ValueOut& o, unsigned char* in_view_out,
                     double* Hc_out, double* elapsed_ms) {
    char* ws = d->value.as<char>();
    const size_t n = (size_t)pl.count;
    d->flush_pending();
    ekf::launch_dense64_value(pl, d->S, d->ld, ws, d->stream);
    return finish_timed(d, elapsed_ms, {{o.dtrace, ws + pl.off_dtrace, sizeof(double) * n},
                                        {o.dtrace_pose, ws + pl.off_dpose, sizeof(double) * n},
                                        {o.detS, ws + pl.off_det, sizeof(double) * n},
                                        {o.S, ws + pl.off_S, sizeof(double) * 4 * n},
                                        {o.flag, ws + pl.off_flag, sizeof(int) * n},
                                        {o.best, ws + pl.off_best, sizeof(ekf_dense64_value_best)},
                                        {in_view_out, ws + pl.off_view, n},
                                        {Hc_out, ws + pl.off_Hc, sizeof(double) * 10 * n}});
}
}  // namespace

ekf_status ekf_dense64_value_operands(ekf_dense64_handle d, int first_lm, int count, const double* Hc, const double* R,
                                      const unsigned char* in_view, double* dtrace, double* dtrace_pose, double* detS,
                                      double* S_out, int* flag_out, ekf_dense64_value_best* best, double* elapsed_ms) {
    const char* fnc = "ekf_dense64_value_operands";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fnc) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    const ValueOut o{dtrace, dtrace_pose, detS, S_out, flag_out, best};
    EKFC(value_checks(d, fnc, first_lm, count, !o.none()));
    if (!Hc || !R) return fail(EKF_ERR_INVALID, std::string(fnc) + ": null Hc or R");
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64ValuePlan pl = ekf::dense64_value_plan(d->live, first_lm, count);
    EKFC(d->value.reserve(d->mem, pl.bytes, false, fnc, "the observation values' workspace"));
    char* ws = d->value.as<char>();
    HIPC(hipMemcpyAsync(ws + pl.off_Hc, Hc, sizeof(double) * 10 * count, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(ws + pl.off_R, R, sizeof(double) * 4, hipMemcpyHostToDevice, d->stream));
    if (in_view) HIPC(hipMemcpyAsync(ws + pl.off_view, in_view, (size_t)count, hipMemcpyHostToDevice, d->stream));
    else HIPC(hipMemsetAsync(ws + pl.off_view, 1, (size_t)count, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    ekf::launch_dense64_value_cols(pl, ws, d->stream);
    return value_run(d, pl, o, nullptr, nullptr, elapsed_ms);
}

ekf_status ekf_dense64_rank_landmarks(ekf_dense64_handle d, const ekf_params* params, int first_lm, int count,
                                      double range_max, double* dtrace, double* dtrace_pose, double* detS, double* S_out,
                                      int* flag_out, ekf_dense64_value_best* best, unsigned char* in_view_out,
                                      double* Hc_out, double* elapsed_ms) {
    const char* fnc = "ekf_dense64_rank_landmarks";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fnc) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    const ValueOut o{dtrace, dtrace_pose, detS, S_out, flag_out, best};
    EKFC(value_checks(d, fnc, first_lm, count, !o.none() || in_view_out || Hc_out));
    const ekf::Params p = landmark_params(params);
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64ValuePlan pl = ekf::dense64_value_plan(d->live, first_lm, count);
    EKFC(d->value.reserve(d->mem, pl.bytes, false, fnc, "the observation values' workspace"));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->finish_leave();   // (a region that is being left ends here: its global update moves the state the terms are built from)
    ekf::launch_dense64_value_terms(pl, d->x, p.r_meas, range_max, d->value.p, d->stream);
    return value_run(d, pl, o, in_view_out, Hc_out, elapsed_ms);
}

// ---- the Cholesky factor of the live corner and the substitution against it (ekf_dense64_factor.hip) ----------------------
ekf_status ekf_dense64_factor_launch_info(ekf_dense64_handle d, int* block, int* threads) {
    if (!d || !block || !threads) return fail(EKF_ERR_INVALID, "ekf_dense64_factor_launch_info: null argument");
    *block = ekf::kDense64FactorNB;
    *threads = ekf::kDense64FactorThreads;
    return EKF_OK;
}

// The buffers are reserved and the verdict word zeroed, the pending rows applied, the chain of launches; the records and the
// diagonal of L come back behind the one synchronisation, and the host folds them in ascending order.
ekf_status ekf_dense64_factor(ekf_dense64_handle d, ekf_dense64_factor_report* out, double* elapsed_ms) {
    const char* fn = "ekf_dense64_factor";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!out) return fail(EKF_ERR_INVALID, std::string(fn) + ": null report");
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64FactorPlan pl = ekf::dense64_factor_plan(d->live);
    EKFC(d->factor_ws.reserve(d->mem, pl.bytes, false, fn, "the factor's records"));
    EKFC(d->factor.reserve(d->mem, pl.factor_bytes, true, fn, "the factor's snapshot"));
    char* ws = d->factor_ws.as<char>();
    HIPC(hipMemsetAsync(ws + pl.off_verdict, 0, sizeof(int), d->stream));
    d->factor_ok = 0;   // the snapshot is being overwritten
    d->factor_na = pl.Na;
    std::vector<ekf::Dense64FactorRecord> rec(pl.blocks);
    std::vector<double> diag(pl.Na);
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    ekf::launch_dense64_factor(pl, d->S, d->ld, d->factor.as<double>(), ws, d->stream);
    EKFC(finish_timed(d, elapsed_ms, {{rec.data(), ws + pl.off_rec, sizeof(ekf::Dense64FactorRecord) * rec.size()},
                                      {diag.data(), ws + pl.off_diag, sizeof(double) * diag.size()}}));
    *out = ekf_dense64_factor_report{};
    out->ok = 1, out->fail_index = -1, out->min_pivot_i = -1, out->Na = pl.Na;
    out->min_pivot = HUGE_VAL, out->max_pivot = 0.0;
    for (const ekf::Dense64FactorRecord& r : rec) {   // ascending: the records behind a failed block were never written
        if (r.min_i >= 0 && r.min_pivot < out->min_pivot) out->min_pivot = r.min_pivot, out->min_pivot_i = r.min_i;
        if (r.max_pivot > out->max_pivot) out->max_pivot = r.max_pivot;
        if (r.fail_index >= 0) {
            out->ok = 0, out->fail_index = r.fail_index, out->fail_pivot = r.fail_pivot;
            break;
        }
    }
    if (out->ok) {
        double sum = 0.0;
        for (int j = 0; j < pl.Na; j++) sum += std::log(diag[j]);
        out->logdet = 2.0 * sum;
    } else {
        out->logdet = std::numeric_limits<double>::quiet_NaN();
    }
    d->factor_ok = out->ok;
    return EKF_OK;
}

namespace {
ekf_status factor_usable(ekf_dense64_s* d, const char* fn, bool same_live) {
    if (!d->factor_ok)
        return fail(EKF_ERR_STATE, std::string(fn) + ": there is no complete factor (no ekf_dense64_factor yet, or the last one ended with ok == 0)");
    if (same_live && d->factor_na != d->live)
        return fail(EKF_ERR_STATE, std::string(fn) + ": the factor was taken at another live dimension");
    return EKF_OK;
}
}  // namespace

ekf_status ekf_dense64_get_factor(ekf_dense64_handle d, double* L_out) {
    const char* fn = "ekf_dense64_get_factor";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    if (!L_out) return fail(EKF_ERR_INVALID, std::string(fn) + ": null output");
    EKFC(factor_usable(d, fn, false));
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64FactorPlan pl = ekf::dense64_factor_plan(d->factor_na);
    const size_t Na = pl.Na;
    HIPC(hipStreamSynchronize(d->stream));
    HIPC(hipMemcpy2D(L_out, sizeof(double) * Na, d->factor.p, sizeof(double) * pl.ldf, sizeof(double) * Na, Na, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < Na; i++)   // whatever the snapshot holds above the diagonal
        for (size_t j = i + 1; j < Na; j++) L_out[i * Na + j] = 0.0;
    return EKF_OK;
}

// The working copy is zeroed and B goes up; one launch per block column and the norms; d2 and Y come back.
ekf_status ekf_dense64_whiten(ekf_dense64_handle d, int nrhs, const double* B, double* Y_out, double* d2_out, double* elapsed_ms) {
    const char* fn = "ekf_dense64_whiten";
    constexpr int kMaxRhs = ekf::kDense64WhitenMaxRhs;
    static_assert(kMaxRhs == EKF_DENSE64_WHITEN_MAX_RHS, "the header's limit");
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    if (!B) return fail(EKF_ERR_INVALID, std::string(fn) + ": null B");
    if (nrhs < 1 || nrhs > kMaxRhs) return fail(EKF_ERR_INVALID, std::string(fn) + ": 1 <= nrhs <= EKF_DENSE64_WHITEN_MAX_RHS");
    if (!Y_out && !d2_out) return fail(EKF_ERR_INVALID, std::string(fn) + ": Y_out and d2_out are both NULL");
    EKFC(factor_usable(d, fn, true));
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64FactorPlan pl = ekf::dense64_factor_plan(d->factor_na);
    const size_t Na = pl.Na, panel = sizeof(double) * kMaxRhs * (size_t)pl.rows, pitch = sizeof(double) * pl.rows;
    EKFC(d->whiten.reserve(d->mem, 2 * panel + sizeof(double) * kMaxRhs, false, fn, "the right-hand sides"));
    double* rhs = d->whiten.as<double>();
    double* d2 = rhs + 2 * (size_t)kMaxRhs * pl.rows;
    HIPC(hipMemsetAsync(rhs, 0, panel, d->stream));
    HIPC(hipMemcpy2DAsync(rhs, pitch, B, sizeof(double) * Na, sizeof(double) * Na, nrhs, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    ekf::launch_dense64_whiten(pl, d->factor.as<double>(), rhs, d2, d->stream);
    EKFC(finish_timed(d, elapsed_ms, {{d2_out, d2, sizeof(double) * nrhs}}));
    if (Y_out)
        HIPC(hipMemcpy2D(Y_out, sizeof(double) * Na, rhs + (size_t)kMaxRhs * pl.rows, pitch, sizeof(double) * Na, nrhs,
                         hipMemcpyDeviceToHost));
    return EKF_OK;
}

ekf_status ekf_dense64_solve_launch_info(ekf_dense64_handle d, int* block, int* threads_back, int* threads_color) {
    if (!d || !block || !threads_back || !threads_color) return fail(EKF_ERR_INVALID, "ekf_dense64_solve_launch_info: null argument");
    *block = ekf::kDense64FactorNB;
    *threads_back = *threads_color = ekf::kDense64FactorThreads;
    return EKF_OK;
}

// ekf_dense64_whiten as it stands on the first two panels, then Y into a third one and the descending walk; X lands where
// the working copy of B was.
ekf_status ekf_dense64_solve(ekf_dense64_handle d, int nrhs, const double* B, double* X_out, double* Y_out, double* d2_out,
                             double* elapsed_ms) {
    const char* fn = "ekf_dense64_solve";
    constexpr int kMaxRhs = ekf::kDense64WhitenMaxRhs;
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    if (!B) return fail(EKF_ERR_INVALID, std::string(fn) + ": null B");
    if (nrhs < 1 || nrhs > kMaxRhs) return fail(EKF_ERR_INVALID, std::string(fn) + ": 1 <= nrhs <= EKF_DENSE64_WHITEN_MAX_RHS");
    if (!X_out && !Y_out && !d2_out) return fail(EKF_ERR_INVALID, std::string(fn) + ": X_out, Y_out and d2_out are all NULL");
    EKFC(factor_usable(d, fn, true));
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64FactorPlan pl = ekf::dense64_factor_plan(d->factor_na);
    const size_t Na = pl.Na, count = kMaxRhs * (size_t)pl.rows, panel = sizeof(double) * count, pitch = sizeof(double) * pl.rows;
    EKFC(d->whiten.reserve(d->mem, 3 * panel + sizeof(double) * kMaxRhs, false, fn, "the right-hand sides"));
    double* rhs = d->whiten.as<double>();   // B, then X | Y | the working copy of Y | d2
    double* d2 = rhs + 3 * count;
    HIPC(hipMemsetAsync(rhs, 0, panel, d->stream));
    HIPC(hipMemcpy2DAsync(rhs, pitch, B, sizeof(double) * Na, sizeof(double) * Na, nrhs, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    ekf::launch_dense64_whiten(pl, d->factor.as<double>(), rhs, d2, d->stream);
    if (X_out) {
        HIPC(hipMemcpyAsync(rhs + 2 * count, rhs + count, panel, hipMemcpyDeviceToDevice, d->stream));
        ekf::launch_dense64_back(pl, d->factor.as<double>(), rhs + 2 * count, rhs, d->stream);
    }
    EKFC(finish_timed(d, elapsed_ms, {{d2_out, d2, sizeof(double) * nrhs}}));
    if (Y_out) HIPC(hipMemcpy2D(Y_out, sizeof(double) * Na, rhs + count, pitch, sizeof(double) * Na, nrhs, hipMemcpyDeviceToHost));
    if (X_out) HIPC(hipMemcpy2D(X_out, sizeof(double) * Na, rhs, pitch, sizeof(double) * Na, nrhs, hipMemcpyDeviceToHost));
    return EKF_OK;
}

// Z goes up into a zeroed panel of the snapshot's row stride, one launch, X comes back.
ekf_status ekf_dense64_color(ekf_dense64_handle d, int nrhs, const double* Z, int add_state, double* X_out, double* elapsed_ms) {
    const char* fn = "ekf_dense64_color";
    constexpr int kMaxRhs = ekf::kDense64WhitenMaxRhs;
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    if (!Z) return fail(EKF_ERR_INVALID, std::string(fn) + ": null Z");
    if (nrhs < 1 || nrhs > kMaxRhs) return fail(EKF_ERR_INVALID, std::string(fn) + ": 1 <= nrhs <= EKF_DENSE64_WHITEN_MAX_RHS");
    if (!X_out) return fail(EKF_ERR_INVALID, std::string(fn) + ": null X_out");
    EKFC(factor_usable(d, fn, true));
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64FactorPlan pl = ekf::dense64_factor_plan(d->factor_na);
    const size_t Na = pl.Na, count = kMaxRhs * (size_t)pl.ldf, panel = sizeof(double) * count, pitch = sizeof(double) * pl.ldf;
    EKFC(d->whiten.reserve(d->mem, 2 * panel, false, fn, "the draws"));
    double* zin = d->whiten.as<double>();   // Z | X
    HIPC(hipMemsetAsync(zin, 0, panel, d->stream));
    HIPC(hipMemcpy2DAsync(zin, pitch, Z, sizeof(double) * Na, sizeof(double) * Na, nrhs, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    ekf::launch_dense64_color(pl, d->factor.as<double>(), zin, add_state ? d->x : nullptr, zin + count, d->stream);
    EKFC(finish_timed(d, elapsed_ms));
    HIPC(hipMemcpy2D(X_out, sizeof(double) * Na, zin + count, pitch, sizeof(double) * Na, nrhs, hipMemcpyDeviceToHost));
    return EKF_OK;
}

// ---- the map in another frame (ekf_dense64_frame.hip) ---------------------------------------------------------------------
ekf_status ekf_dense64_frame_launch_info(ekf_dense64_handle d, int* tile_rows, int* tile_cols, int* threads) {
    if (!d || !tile_rows || !tile_cols || !threads) return fail(EKF_ERR_INVALID, "ekf_dense64_frame_launch_info: null argument");
    *tile_rows = ekf::kDense64FrameTileRows;
    *tile_cols = ekf::kDense64FrameTileCols;
    *threads = ekf::kDense64FrameThreads;
    return EKF_OK;
}

namespace {
static_assert(ekf::kDense64FrameFixed == EKF_DENSE64_FRAME_FIXED && ekf::kDense64FrameRobot == EKF_DENSE64_FRAME_ROBOT,
              "the header's modes");
// the live dimension a frame change runs at (odd, >= 3) and the workspace for it; before e0, nothing changed on a refusal
ekf_status frame_reserve(ekf_dense64_s* d, const char* fn, ekf::Dense64FramePlan* pl) {
    if (d->live < 3 || d->live % 2 == 0)
        return fail(EKF_ERR_INVALID, std::string(fn) + ": the live dimension must be 3 + 2 n (a pose and whole landmarks)");
    HIPC(hipSetDevice(d->device));
    *pl = ekf::dense64_frame_plan(d->live, d->ld);
    return d->frame.reserve(d->mem, sizeof(double) * pl->doubles, false, fn, "the frame change's workspace");
}
// G = I in bits (+1, +0, +0, +1): with no C the congruence is the identity map and Sigma is not passed over
bool is_identity(const double* G) {
    const double I[4] = {1.0, 0.0, 0.0, 1.0};
    return std::memcmp(G, I, sizeof(I)) == 0;
}
}  // namespace

// G and C go up into the terms region, the pending rows are applied, three launches.
ekf_status ekf_dense64_map_congruence(ekf_dense64_handle d, const double* G, const double* C, double* elapsed_ms) {
    const char* fn = "ekf_dense64_map_congruence";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!G) return fail(EKF_ERR_INVALID, std::string(fn) + ": null G");
    ekf::Dense64FramePlan pl;
    EKFC(frame_reserve(d, fn, &pl));
    double* ws = d->frame.as<double>();
    HIPC(hipMemcpyAsync(ws + pl.off_terms, G, sizeof(double) * 4, hipMemcpyHostToDevice, d->stream));
    if (C) HIPC(hipMemcpyAsync(ws + pl.off_terms + 4, C, sizeof(double) * 3 * (size_t)pl.Na, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    if (C || !is_identity(G)) ekf::launch_dense64_frame_congruence(pl, d->S, ws, C != nullptr, d->stream);
    return finish_timed(d, elapsed_ms);
}

// One launch for the terms and the new state, the congruence on those terms, the new state copied over the old one.
ekf_status ekf_dense64_reframe_landmarks(ekf_dense64_handle d, int mode, double dtheta, double tx, double ty, double* terms_out,
                                         double* elapsed_ms) {
    const char* fn = "ekf_dense64_reframe_landmarks";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (mode != EKF_DENSE64_FRAME_FIXED && mode != EKF_DENSE64_FRAME_ROBOT)
        return fail(EKF_ERR_INVALID, std::string(fn) + ": mode is EKF_DENSE64_FRAME_FIXED or EKF_DENSE64_FRAME_ROBOT");
    const bool robot = mode == EKF_DENSE64_FRAME_ROBOT;
    if (!robot && !(std::isfinite(dtheta) && std::isfinite(tx) && std::isfinite(ty)))
        return fail(EKF_ERR_INVALID, std::string(fn) + ": dtheta, tx and ty must be finite");
    ekf::Dense64FramePlan pl;
    EKFC(frame_reserve(d, fn, &pl));
    double* ws = d->frame.as<double>();
    const double c = robot ? 0.0 : std::cos(dtheta), s = robot ? 0.0 : std::sin(dtheta);
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    ekf::launch_dense64_frame_state(pl, mode, d->x, ws, dtheta, c, s, tx, ty, d->stream);
    ekf::launch_dense64_frame_congruence(pl, d->S, ws, robot, d->stream);
    HIPC(hipMemcpyAsync(d->x, ws + pl.off_state, sizeof(double) * pl.Na, hipMemcpyDeviceToDevice, d->stream));
    if (terms_out && !robot) std::fill(terms_out + 4, terms_out + 4 + 3 * (size_t)pl.Na, 0.0);   // (no C was used)
    return finish_timed(d, elapsed_ms, {{terms_out, ws + pl.off_terms, sizeof(double) * (robot ? 4 + 3 * (size_t)pl.Na : 4)}});
}

// ---- map joining (ekf_dense64_join.hip) -------------------------------------------------------------------------------------
ekf_status ekf_dense64_join_launch_info(ekf_dense64_handle d, int* tile_rows, int* tile_cols, int* threads) {
    if (!d || !tile_rows || !tile_cols || !threads) return fail(EKF_ERR_INVALID, "ekf_dense64_join_launch_info: null argument");
    *tile_rows = ekf::kDense64JoinTileRows;
    *tile_cols = ekf::kDense64JoinTileCols;
    *threads = ekf::kDense64JoinThreads;
    return EKF_OK;
}

namespace {
// Both calls: the refusals in the header's order (host only: a region that either handle is in stays open when one strikes),
// the workspace from the destination's ledger, then behind the destination's e0 its pending rows, the source's on the
// source's own stream with an event the destination's stream waits on, the launches, and the new live dimension.
// map: G and E are built on the device and the state goes along; otherwise they go up from the caller.
ekf_status dense64_join(const char* fnc, ekf_dense64_s* dst, ekf_dense64_s* src, bool map, const double* G, const double* E,
                        double* terms_out, double* elapsed_ms) {
    const std::string fn = fnc;
    if (!dst) return fail(EKF_ERR_INVALID, fn + ": null destination handle");
    if (!src) return fail(EKF_ERR_INVALID, fn + ": null source handle");
    if (dst == src) return fail(EKF_ERR_INVALID, fn + ": the destination and the source are the same handle");
    if (dst->device != src->device) return fail(EKF_ERR_INVALID, fn + ": the two handles live on different devices");
    const RegionLeave leaving_dst(dst), leaving_src(src);   // outside a region's terms: it ends behind the checks and e0
    const int Na = dst->live, Nb = src->live;
    if (Na < 3 || Na % 2 == 0 || Nb < 3 || Nb % 2 == 0)
        return fail(EKF_ERR_INVALID, fn + ": both live dimensions must be 3 + 2 n (a pose and whole landmarks)");
    if ((long long)Na + Nb - 3 > dst->N)
        return fail(EKF_ERR_INVALID, fn + ": the joined map (Na + Nb - 3 states) does not fit the destination's N");
    if (!map && (!G || !E)) return fail(EKF_ERR_INVALID, fn + ": null G or E");
    HIPC(hipSetDevice(dst->device));
    const ekf::Dense64JoinPlan pl = ekf::dense64_join_plan(Na, dst->ld, Nb, src->ld);
    EKFC(dst->join.reserve(dst->mem, sizeof(double) * pl.doubles, false, fnc, "the join's workspace"));
    double* ws = dst->join.as<double>();
    const size_t terms_bytes = sizeof(double) * (4 + 3 * (size_t)Nb);
    if (!map) {
        HIPC(hipMemcpyAsync(ws + pl.off_terms, G, sizeof(double) * 4, hipMemcpyHostToDevice, dst->stream));
        HIPC(hipMemcpyAsync(ws + pl.off_terms + 4, E, terms_bytes - sizeof(double) * 4, hipMemcpyHostToDevice, dst->stream));
    }
    HIPC(hipEventRecord(dst->e0, dst->stream));
    dst->flush_pending();
    src->sigma_needed();   // (on the source's stream)
    HIPC(hipEventRecord(src->e1, src->stream));
    HIPC(hipStreamWaitEvent(dst->stream, src->e1, 0));
    if (map) ekf::launch_dense64_join_state(pl, dst->x, src->x, ws, dst->stream);
    ekf::launch_dense64_join_congruence(pl, dst->S, src->S, ws, dst->stream);
    if (map) HIPC(hipMemcpyAsync(dst->x, ws + pl.off_pose, sizeof(double) * 3, hipMemcpyDeviceToDevice, dst->stream));
    EKFC(finish_timed(dst, elapsed_ms, {{map ? terms_out : nullptr, ws + pl.off_terms, terms_bytes}}));
    dst->live = pl.Nj;   // (no rows are pending: nothing to widen)
    dst->pl_live = ekf::dense64_live_plan(dst->pl_full, dst->live);
    return EKF_OK;
}
}  // namespace

ekf_status ekf_dense64_join_congruence(ekf_dense64_handle dst, ekf_dense64_handle src, const double* G, const double* E,
                                       double* elapsed_ms) {
    return dense64_join("ekf_dense64_join_congruence", dst, src, false, G, E, nullptr, elapsed_ms);
}

ekf_status ekf_dense64_join_map(ekf_dense64_handle dst, ekf_dense64_handle src, double* terms_out, double* elapsed_ms) {
    return dense64_join("ekf_dense64_join_map", dst, src, true, nullptr, nullptr, terms_out, elapsed_ms);
}

// ---- a map or a submap copied into a second handle (ekf_dense64_extract.hip) ------------------------------------------------
ekf_status ekf_dense64_extract_launch_info(ekf_dense64_handle d, int* tile_rows, int* tile_cols, int* threads) {
    if (!d || !tile_rows || !tile_cols || !threads)
        return fail(EKF_ERR_INVALID, "ekf_dense64_extract_launch_info: null argument");
    *tile_rows = ekf::kDense64ExtractTileRows;
    *tile_cols = ekf::kDense64ExtractTileCols;
    *threads = ekf::kDense64ExtractThreads;
    return EKF_OK;
}

// The refusals in the header's order (host only: a region that either handle is in stays open when one strikes), the list
// with its run flags into the workspace from the destination's ledger, the destination's panels if the source has rows
// pending and the destination has none; then behind the destination's e0 its own region end and pending rows, the source's
// region end on the source's stream with an event the destination's stream waits on, the launches, and the destination's
// new live dimension and pending count.  The source's pending rows are neither applied nor counted down.
ekf_status ekf_dense64_extract_map(ekf_dense64_handle dst, ekf_dense64_handle src, int k, const int* keep, double* elapsed_ms) {
    const char* fnc = "ekf_dense64_extract_map";
    const std::string fn = fnc;
    if (!dst) return fail(EKF_ERR_INVALID, fn + ": null destination handle");
    if (!src) return fail(EKF_ERR_INVALID, fn + ": null source handle");
    if (dst == src) return fail(EKF_ERR_INVALID, fn + ": the destination and the source are the same handle");
    if (dst->device != src->device) return fail(EKF_ERR_INVALID, fn + ": the two handles live on different devices");
    const RegionLeave leaving_dst(dst), leaving_src(src);   // outside a region's terms: it ends behind the checks and e0
    const int Nb = src->live;
    if (Nb < 3 || Nb % 2 == 0)
        return fail(EKF_ERR_INVALID, fn + ": the source's live dimension must be 3 + 2 b (a pose and whole landmarks)");
    const int b = (Nb - 3) / 2;
    if (keep ? k < 0 : (k != -1 && k != b))
        return fail(EKF_ERR_INVALID, fn + ": k must be >= 0, and with a null list b (the source's landmarks) or -1");
    if (!keep) k = b;
    if (keep) {
        for (int t = 0; t < k; t++)
            if (keep[t] < 0 || keep[t] >= b)
                return fail(EKF_ERR_INVALID, fn + ": every index of keep must be a landmark of the source, in [0, b)");
        std::vector<int>& stamp = dst->host_stamp;
        stamp.assign(b, 0);
        for (int t = 0; t < k; t++)
            if (stamp[keep[t]]++) return fail(EKF_ERR_INVALID, fn + ": keep names a landmark twice");
    }
    if (3 + 2 * (long long)k > dst->N)
        return fail(EKF_ERR_INVALID, fn + ": the extracted map (3 + 2 k states) does not fit the destination's N");
    HIPC(hipSetDevice(dst->device));
    const ekf::Dense64ExtractPlan pl = ekf::dense64_extract_plan(Nb, src->ld, k, dst->ld);
    const int p = src->region_leaving ? 0 : src->pend_rows;   // (a region's end applies the rows it finds)
    EKFC(dst->extract.reserve(dst->mem, sizeof(int) * pl.ints, false, fnc, "the extraction's list"));
    if (p > 0) EKFC(pend_reserve(dst, fnc));
    std::vector<int>& up = dst->host_keep;   // the list | per column tile: its landmarks are a contiguous ascending run
    up.assign(pl.ints, 0);
    for (int t = 0; t < k; t++) up[pl.off_keep + t] = keep ? keep[t] : t;
    constexpr int kLc = ekf::kDense64ExtractTileCols / 2;
    for (int c = 0; c < pl.corner_gx; c++) {
        const int* first = up.data() + pl.off_keep + (size_t)c * kLc;
        const int n = std::min(kLc, k - c * kLc);
        int l = 1;
        while (l < n && first[l] == first[0] + l) l++;
        up[pl.off_run + c] = l == n;
    }
    int* ws = dst->extract.as<int>();
    HIPC(hipMemcpyAsync(ws, up.data(), sizeof(int) * pl.ints, hipMemcpyHostToDevice, dst->stream));
    HIPC(hipEventRecord(dst->e0, dst->stream));
    dst->flush_pending();   // the destination is overwritten: its region ends, its own rows are applied
    src->finish_leave();    // (on the source's stream; nothing when no region is open: its rows stay pending)
    HIPC(hipEventRecord(src->e1, src->stream));
    HIPC(hipStreamWaitEvent(dst->stream, src->e1, 0));
    ekf::launch_dense64_extract(pl, dst->S, dst->x, src->S, src->x, ws, dst->stream);
    if (p > 0) {
        const PendView from = src->panels(), to = dst->panels();
        ekf::launch_dense64_extract_panels(pl, to.K, to.T, from.K, from.T, p, ws, dst->stream);
    }
    EKFC(finish_timed(dst, elapsed_ms));
    dst->live = pl.Nd;
    dst->pl_live = ekf::dense64_live_plan(dst->pl_full, dst->live);
    dst->pend_rows = p;
    return EKF_OK;
}

// ---- duplicate landmarks: the all-pairs scan (ekf_dense64_pairs.hip) and the merge, a layer over the calls above ----------
ekf_status ekf_dense64_pairs_launch_info(ekf_dense64_handle d, int* tile_landmarks, int* threads) {
    if (!d || !tile_landmarks || !threads) return fail(EKF_ERR_INVALID, "ekf_dense64_pairs_launch_info: null argument");
    *tile_landmarks = ekf::kDense64PairsTile;
    *threads = ekf::kDense64PairsThreads;
    return EKF_OK;
}

// The counters are zeroed, the pending rows applied, two launches; nearest, d2 and the two counts come back behind the one
// synchronisation.  The workspace grows with n_lm and is the only thing the call changes in the handle.
ekf_status ekf_dense64_score_landmark_pairs(ekf_dense64_handle d, int n_lm, double r_merge, double gate, int* nearest,
                                            double* d2, long long* n_below, long long* n_flagged, double* elapsed_ms) {
    const char* fn = "ekf_dense64_score_landmark_pairs";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!nearest && !d2) return fail(EKF_ERR_INVALID, std::string(fn) + ": nearest and d2 are both NULL");
    if (n_lm < 1 || 3 + 2 * (long long)n_lm > d->live)
        return fail(EKF_ERR_INVALID, std::string(fn) + ": the n_lm >= 1 landmarks must lie inside the live dimension");
    if (!(r_merge >= 0.0) || !std::isfinite(r_merge) || gate != gate)
        return fail(EKF_ERR_INVALID, std::string(fn) + ": r_merge must be finite and >= 0, gate not a NaN");
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64PairsPlan pl = ekf::dense64_pairs_plan(n_lm);
    EKFC(d->pairs.reserve(d->mem, pl.bytes, false, fn, "the pair scan's workspace"));
    char* ws = d->pairs.as<char>();
    unsigned long long counts[2] = {0, 0};
    HIPC(hipMemsetAsync(ws + pl.off_count, 0, sizeof(counts), d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->flush_pending();
    ekf::launch_dense64_pairs(pl, d->S, d->x, d->ld, r_merge, gate, ws, d->stream);
    EKFC(finish_timed(d, elapsed_ms, {{nearest, ws + pl.off_nearest, sizeof(int) * n_lm},
                                      {d2, ws + pl.off_d2, sizeof(double) * n_lm},
                                      {counts, ws + pl.off_count, sizeof(counts)}}));
    if (n_below) *n_below = (long long)counts[0];
    if (n_flagged) *n_flagged = (long long)counts[1];
    return EKF_OK;
}

// The removal of landmark i of *known ("Removing a landmark") -- through the public calls, so that carry,
// pending rows and live behave as in the spelled sequence --: [swap_blocks] init_block [set_live].  Shared by the merge and
// by ekf_dense64_remove_landmark; the arguments are the caller's to check.
namespace {
ekf_status remove_landmark_legs(ekf_dense64_s* d, const ekf::Params& p, int i, int* known, bool shrink, int* moved_from,
                                LegTimer& leg) {
    const int last = *known - 1;
    double* pms = leg.pms();
    const double W[4] = {p.sigma0_landmark, 0.0, 0.0, p.sigma0_landmark};
    if (i != last) EKFC(leg(ekf_dense64_swap_blocks(d, 3 + 2 * i, 3 + 2 * last, 2, pms)));
    EKFC(leg(ekf_dense64_init_block(d, 3 + 2 * last, 2, 0, nullptr, nullptr, W, nullptr, pms)));
    *known = last;
    if (moved_from) *moved_from = i != last ? last : -1;
    if (shrink) EKFC(ekf_dense64_set_live(d, 3 + 2 * last));
    return EKF_OK;
}
}  // namespace

// [terms | the sparse correction, eager or deferred] and its synchronisation, then the removal of hi.
ekf_status ekf_dense64_merge_landmarks(ekf_dense64_handle d, const ekf_params* params, int a, int b, double r_merge,
                                       int* known, int flags, int* moved_from, double* d2_out, double* elapsed_ms) {
    const char* fnc = "ekf_dense64_merge_landmarks";
    const std::string fn = fnc;
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!known) return fail(EKF_ERR_INVALID, fn + ": null argument");
    if (*known < 0 || 3 + 2 * (long long)*known > d->live)
        return fail(EKF_ERR_INVALID, fn + ": the known landmarks must lie inside the live dimension");
    if (a == b || a < 0 || b < 0 || a >= *known || b >= *known)
        return fail(EKF_ERR_INVALID, fn + ": a and b must be two different landmarks in [0, *known)");
    if (!(r_merge >= 0.0) || !std::isfinite(r_merge)) return fail(EKF_ERR_INVALID, fn + ": r_merge must be finite and >= 0");
    EKFC(lm_flags_ok(fn, (unsigned)flags, EKF_DENSE64_LM_DEFERRED | EKF_DENSE64_LM_GROW_LIVE | EKF_DENSE64_LM_JOSEPH));
    const bool deferred = (flags & EKF_DENSE64_LM_DEFERRED) != 0;
    const ekf::Params p = landmark_params(params);
    const int lo = std::min(a, b), hi = std::max(a, b);
    if (elapsed_ms) *elapsed_ms = 0.0;
    HIPC(hipSetDevice(d->device));
    if (deferred) EKFC(pend_reserve(d, fnc));
    const CorrSparseView cin = view(d->corr_in, L::corr_sparse_layout(d->ld));
    LegTimer leg(elapsed_ms);
    double* pms = leg.pms();
    HIPC(hipEventRecord(d->e0, d->stream));
    d->finish_leave();   // (a region that is being left ends here)
    ekf::launch_dense64_pair_terms(d->x, lo, hi, r_merge, cin.cols, cin.Hc, cin.R, cin.nu, d->stream);
    correct_sparse_launch(d, deferred, 2, 4, true, lm_joseph((unsigned)flags));
    EKFC(leg(correct_sparse_finish(d, fnc, deferred, 2, d2_out, pms)));   // singular: nothing was written, *known stands
    return remove_landmark_legs(d, p, hi, known, (flags & EKF_DENSE64_LM_GROW_LIVE) != 0, moved_from, leg);
}

// The removal alone.  Inside an open region the three calls behave as they do when the caller spells them.
ekf_status ekf_dense64_remove_landmark(ekf_dense64_handle d, const ekf_params* params, int i, int* known, unsigned flags,
                                       int* moved_from, double* elapsed_ms) {
    const std::string fn = "ekf_dense64_remove_landmark";
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    if (!known) return fail(EKF_ERR_INVALID, fn + ": null argument");
    if (*known < 0 || 3 + 2 * (long long)*known > d->live)
        return fail(EKF_ERR_INVALID, fn + ": the known landmarks must lie inside the live dimension");
    if (i < 0 || i >= *known) return fail(EKF_ERR_INVALID, fn + ": i must be a landmark in [0, *known)");
    EKFC(lm_flags_ok(fn, flags, EKF_DENSE64_LM_GROW_LIVE));
    const ekf::Params p = landmark_params(params);
    if (elapsed_ms) *elapsed_ms = 0.0;
    LegTimer leg(elapsed_ms);
    return remove_landmark_legs(d, p, i, known, (flags & EKF_DENSE64_LM_GROW_LIVE) != 0, moved_from, leg);
}

// ---- a scan cast against the map: evidence for and against landmarks (ekf_dense64_evidence.hip, ekf_dense64_evidence.hpp) --
ekf_status ekf_dense64_evidence_launch_info(ekf_dense64_handle d, int* beam_tile, int* lm_chunk, int* threads) {
    if (!d || !beam_tile || !lm_chunk || !threads)
        return fail(EKF_ERR_INVALID, "ekf_dense64_evidence_launch_info: null argument");
    *beam_tile = ekf::kDense64EvidenceBeamTile;
    *lm_chunk = ekf::kDense64EvidenceLmChunk;
    *threads = ekf::kDense64EvidenceThreads;
    return EKF_OK;
}

// The checks in the documented order; the workspace, the ring and (kappa > 0) the candidates' buffer reserved; the ranges up
// through a slot of the ring and the counters zeroed; behind e0 the end of a region that is being left, per chunk of
// landmarks [terms | the sparse scoring kernel, reading through the pending rows | tolerances], the two launches of the cast;
// everything asked for back behind the one synchronisation.
ekf_status ekf_dense64_scan_evidence(ekf_dense64_handle d, const ekf_params* params, const ekf_lidar_params* lidar,
                                     const double* ranges, int first_lm, int count, double tol_abs, double kappa,
                                     int* n_expected, int* n_agree, int* n_through, int* n_short, double* tol_out,
                                     double* expected_out, int* hit_out, unsigned char* class_out,
                                     ekf_dense64_evidence_report* report, double* elapsed_ms) {
    const char* fnc = "ekf_dense64_scan_evidence";
    const std::string fn = fnc;
    if (!d || !lidar) return fail(EKF_ERR_INVALID, fn + ": null handle or lidar");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!n_expected && !n_agree && !n_through && !n_short && !tol_out && !expected_out && !hit_out && !class_out && !report)
        return fail(EKF_ERR_INVALID, fn + ": every output is NULL");
    if (count < 1 || first_lm < 0) return fail(EKF_ERR_INVALID, fn + ": count >= 1 and first_lm >= 0");
    if (3 + 2 * ((long long)first_lm + count) > d->live)
        return fail(EKF_ERR_INVALID, fn + ": the landmarks must lie inside the live dimension");
    const int nb = lidar->n_beams;
    if (nb < 1 || nb > kScanBeams) return fail(EKF_ERR_INVALID, fn + ": n_beams must lie in [1, 1024]");
    if (!std::isfinite(lidar->tube_radius) || !(lidar->tube_radius > 0.0) || !std::isfinite(lidar->range_max) ||
        !(lidar->range_max > 0.0))
        return fail(EKF_ERR_INVALID, fn + ": tube_radius and range_max must be finite and > 0");
    if (!(tol_abs >= 0.0) || !(kappa >= 0.0)) return fail(EKF_ERR_INVALID, fn + ": tol_abs and kappa must be >= 0");
    if (lidar->model != 0) return fail(EKF_ERR_INVALID, fn + ": only the clean ray geometry (model 0) is cast");
    const ekf::Params p = landmark_params(params);
    HIPC(hipSetDevice(d->device));
    const ekf::Dense64EvidencePlan pl = ekf::dense64_evidence_plan(first_lm, count);
    const bool scored = kappa > 0.0;
    const int chunk = std::min(count, kSparseRows / 2);
    EKFC(d->evidence.reserve(d->mem, pl.bytes, false, fnc, "the scan evidence's workspace"));
    if (scored) EKFC(sps_reserve(d, L::sps_layout(chunk, 2, 5, true, true).bytes, fnc));
    char* ws = d->evidence.as<char>();
    if (ranges) {
        for (Staging& sg : d->scan_up.slot) EKFC(sg.reserve(sizeof(double) * kScanBeams));
        Staging& sg = d->scan_up.acquire();
        EKFC(sg.wait());
        std::memcpy(sg.host, ranges, sizeof(double) * nb);
        HIPC(hipMemcpyAsync(ws + pl.off_ranges, sg.host, sizeof(double) * nb, hipMemcpyHostToDevice, d->stream));
        EKFC(sg.mark(d->stream));
    }
    HIPC(hipMemsetAsync(ws + pl.off_report, 0, pl.zero_bytes, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->finish_leave();   // (a region that is being left ends here: its global update moves the landmarks the beams are cast at)
    if (scored) {
        for (int at = 0; at < count; at += chunk) {
            const int n = std::min(chunk, count - at);
            const SpsView v = view(d->sps.p, L::sps_layout(n, 2, 5, true, true), true);
            ekf::launch_dense64_lm_terms(d->x, d->x, 0.0, 0.0, first_lm + at, n, 0, p.r_meas, v.cols, v.Hc, v.R, v.nu,
                                         d->stream);
            score_sparse_launch(d, v, n, 2, 5, true, false, false);   // (S and the flag do not depend on the reading)
            ekf::launch_dense64_evidence_tol(pl, at, n, v.S, v.flag, tol_abs, kappa, ws, d->stream);
        }
    } else {
        ekf::launch_dense64_evidence_tol(pl, 0, count, nullptr, nullptr, tol_abs, kappa, ws, d->stream);
    }
    ekf::launch_dense64_evidence(pl, d->x, nb, lidar->range_max, lidar->border_width, lidar->tube_radius, tol_abs,
                                 ranges != nullptr, ws, d->stream);
    int rep[4] = {0, 0, 0, 0};
    const size_t ci = sizeof(int) * (size_t)count;
    EKFC(finish_timed(d, elapsed_ms, {{rep, ws + pl.off_report, sizeof(rep)},
                                      {n_expected, ws + pl.off_counts, ci},
                                      {n_agree, ws + pl.off_counts + ci, ci},
                                      {n_through, ws + pl.off_counts + 2 * ci, ci},
                                      {n_short, ws + pl.off_counts + 3 * ci, ci},
                                      {tol_out, ws + pl.off_tol, sizeof(double) * count},
                                      {expected_out, ws + pl.off_expected, sizeof(double) * nb},
                                      {hit_out, ws + pl.off_hit, sizeof(int) * nb},
                                      {class_out, ws + pl.off_class, (size_t)nb}}));
    if (report) *report = ekf_dense64_evidence_report{rep[0], rep[1], rep[2], rep[3]};
    return EKF_OK;
}

ekf_status ekf_dense64_evidence_update(int count, const int* n_expected, const int* n_agree, const int* n_through,
                                       int min_beams, double w_hit, double w_miss, double l_min, double l_max,
                                       double* logodds, int* verdict_out) {
    const std::string fn = "ekf_dense64_evidence_update";
    if (!n_expected || !n_agree || !n_through || !logodds) return fail(EKF_ERR_INVALID, fn + ": null argument");
    if (count < 1 || min_beams < 1) return fail(EKF_ERR_INVALID, fn + ": count >= 1 and min_beams >= 1");
    if (!(w_hit >= 0.0) || !(w_miss >= 0.0) || !(l_min <= l_max))
        return fail(EKF_ERR_INVALID, fn + ": w_hit and w_miss must be >= 0 and l_min <= l_max, none of them a NaN");
    ekf::evidence_update(count, n_expected, n_agree, n_through, min_beams, w_hit, w_miss, l_min, l_max, logodds, verdict_out);
    return EKF_OK;
}

// ---- the landmark front end: the reference's model and decision rule on the handle's own state -------------------------
// calculate_maha_dis (:217-276) of one reading: k_dlm_terms writes the operands through the view the uploads of score_sparse
// use, then that call's one launch; everything asked for comes back behind the one synchronisation.
ekf_status ekf_dense64_score_landmarks(ekf_dense64_handle d, const ekf_params* params, double sx, double sy, int first_lm,
                                       int count, double* nis_out, double* S_out, int* flag_out, int* cols_out,
                                       double* Hc_out, double* nu_out, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_score_landmarks: null handle");
    if (count < 1 || count > kSparseRows / 2 || first_lm < 0 || 3 + 2 * ((long long)first_lm + count) > d->live ||
        (!nis_out && !S_out && !flag_out))
        return fail(EKF_ERR_INVALID, "ekf_dense64_score_landmarks: bad argument (the landmarks must lie inside the live "
                                     "dimension)");
    const ekf::Params p = landmark_params(params);
    HIPC(hipSetDevice(d->device));
    const L::SpsLayout l = L::sps_layout(count, 2, 5, true, S_out != nullptr);
    EKFC(sps_reserve(d, l.bytes, "ekf_dense64_score_landmarks"));
    const SpsView v = view(d->sps.p, l, S_out != nullptr);
    HIPC(hipEventRecord(d->e0, d->stream));
    ekf::launch_dense64_lm_terms(d->x, d->x, sx, sy, first_lm, count, 0, p.r_meas, v.cols, v.Hc, v.R, v.nu, d->stream);
    score_sparse_launch(d, v, count, 2, 5, true, true, nis_out != nullptr);
    return finish_timed(d, elapsed_ms, {{nis_out, v.nis, sizeof(double) * count},
                                        {S_out, v.S, sizeof(double) * count * 4},
                                        {flag_out, v.flag, sizeof(int) * count},
                                        {cols_out, v.cols, sizeof(int) * count * 5},
                                        {Hc_out, v.Hc, sizeof(double) * count * 10},
                                        {nu_out, v.nu, sizeof(double) * count * 2}});
}

// data_association (:278-402) for J readings.  Per reading: [terms | score | decide] and the 32-byte record back (the first
// synchronisation); then, as the record says, [init_block] [terms of the winner, wrapped | correction | heading wrap] and
// the correction's own synchronisation.  Nothing of the state comes down and no candidate array goes up.
ekf_status ekf_dense64_associate_landmarks(ekf_dense64_handle d, const ekf_params* params, int J, const double* meas_xy,
                                           int n_max, int* known, unsigned flags, int* assoc_out, double* best_out,
                                           double* elapsed_ms) {
    const AssocRule r{Rule::kSequential, INT_MAX, kLmFlags | EKF_DENSE64_LM_JOSEPH, false};
    return assoc_readings_form(d, "ekf_dense64_associate_landmarks", r, params, J, meas_xy, n_max, known, flags, assoc_out,
                               best_out, nullptr, elapsed_ms);
}

// ---- a laser scan as the handle's input --------------------------------------------------------------------------------
ekf_status ekf_dense64_fit_scan(ekf_dense64_handle d, const double* ranges, int n_beams, int max_out, int* count_out,
                                double* centres_out, double* radii_out, double* all_clusters, int* n_clusters,
                                double* elapsed_ms) {
    const char* fn = "ekf_dense64_fit_scan";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fn) + ": null handle");
    if (!ranges || !count_out) return fail(EKF_ERR_INVALID, std::string(fn) + ": null argument");
    if (n_beams < 1 || n_beams > kScanBeams || max_out < 1 || max_out > kScanClusters)
        return fail(EKF_ERR_INVALID, std::string(fn) + ": n_beams must lie in [1, 1024] and max_out in [1, 128]");
    HIPC(hipSetDevice(d->device));
    ScanRecord rec{};
    EKFC(scan_fit(d, fn, ranges, n_beams, max_out, all_clusters != nullptr, elapsed_ms, &rec));
    *count_out = rec.count;
    if (n_clusters) *n_clusters = rec.n_clusters;
    for (int i = 0; i < max_out; i++) {   // entries beyond the count are zero
        const bool in = i < rec.count;
        if (centres_out) { centres_out[2 * i] = in ? rec.centres[2 * i] : 0.0; centres_out[2 * i + 1] = in ? rec.centres[2 * i + 1] : 0.0; }
        if (radii_out) radii_out[i] = in ? rec.radii[i] : 0.0;
    }
    if (all_clusters)
        for (int i = 0; i < kScanClusters * 4; i++) all_clusters[i] = i < rec.n_clusters * 4 ? rec.all[i] : 0.0;
    return EKF_OK;
}

// ekf_dense64_fit_scan, then the loop of ekf_dense64_associate_landmarks on the first min(count, max_readings) centres
ekf_status ekf_dense64_associate_scan(ekf_dense64_handle d, const ekf_params* params, const double* ranges, int n_beams,
                                      int max_readings, int n_max, int* known, unsigned flags, int* count_out,
                                      double* centres_out, int* assoc_out, double* best_out, double* elapsed_ms) {
    const AssocRule r{Rule::kSequential, INT_MAX, kLmFlags, false};
    return assoc_scan_form(d, "ekf_dense64_associate_scan", r, params, ranges, n_beams, max_readings, n_max, known, flags,
                           count_out, centres_out, assoc_out, best_out, elapsed_ms);
}

// ---- a whole scan at once: every reading against one state, one assignment, one stacked correction ----------------------
// calculate_maha_dis of J readings: the readings go up in one copy, per launch of at most 32768 / count readings the
// candidates' operands and score_sparse's one launch, the outputs queued behind it; ONE synchronisation.
ekf_status ekf_dense64_score_readings(ekf_dense64_handle d, const ekf_params* params, int J, const double* meas_xy,
                                      int first_lm, int count, double* nis_out, int* flag_out, double* elapsed_ms) {
    const char* fnc = "ekf_dense64_score_readings";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fnc) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!meas_xy || J < 1 || J > kJointReadings || count < 1 || count > kSparseRows / 2 || first_lm < 0 ||
        3 + 2 * ((long long)first_lm + count) > d->live || (!nis_out && !flag_out))
        return fail(EKF_ERR_INVALID, std::string(fnc) + ": bad argument (1 <= J <= 128, 1 <= count <= 32768, the landmarks "
                                                        "inside the live dimension)");
    const ekf::Params p = landmark_params(params);
    HIPC(hipSetDevice(d->device));
    EKFC(joint_reserve(d, fnc));
    const int chunk = joint_chunk(J, count);
    EKFC(sps_reserve(d, L::sps_layout(chunk * count, 2, 5, true, false).bytes, fnc));
    const JointView jv = view(d->joint.p, L::joint_layout());
    HIPC(hipMemcpyAsync(jv.xy, meas_xy, sizeof(double) * 2 * J, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->finish_leave();   // (a region that is being left ends here)
    hipError_t queued = hipSuccess;
    score_readings_launch(d, p, jv, J, first_lm, count, chunk, nis_out != nullptr, [&](int j0, int nr, const SpsView& v) {
        const size_t at = (size_t)j0 * count, n = (size_t)nr * count;
        if (j0 + nr == J) return;   // the last launch's outputs come down with finish_timed, behind e1
        if (nis_out && queued == hipSuccess)
            queued = hipMemcpyAsync(nis_out + at, v.nis, sizeof(double) * n, hipMemcpyDeviceToHost, d->stream);
        if (flag_out && queued == hipSuccess)
            queued = hipMemcpyAsync(flag_out + at, v.flag, sizeof(int) * n, hipMemcpyDeviceToHost, d->stream);
    });
    HIPC(queued);
    const int j_last = (J - 1) / chunk * chunk;
    const size_t at = (size_t)j_last * count, n = (size_t)(J - j_last) * count;
    const SpsView v = view(d->sps.p, L::sps_layout(chunk * count, 2, 5, true, false), false);
    return finish_timed(d, elapsed_ms, {{nis_out ? nis_out + at : nullptr, v.nis, sizeof(double) * n},
                                        {flag_out ? flag_out + at : nullptr, v.flag, sizeof(int) * n}});
}

// The stacked operands of V pairs from the current state: the two lists go up, one launch into the sparse correction's
// operand buffer (which every correction fills anew), one synchronisation.  Read-only.
ekf_status ekf_dense64_joint_operands(ekf_dense64_handle d, const ekf_params* params, int V, const int* lm_idx,
                                      const double* meas_xy, int* cols_out, double* Hc_out, double* nu_out,
                                      double* elapsed_ms) {
    const char* fnc = "ekf_dense64_joint_operands";
    if (!d) return fail(EKF_ERR_INVALID, std::string(fnc) + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!lm_idx || !meas_xy || V < 1 || V > kJointPairs || (!cols_out && !Hc_out && !nu_out))
        return fail(EKF_ERR_INVALID, std::string(fnc) + ": bad argument (1 <= V <= 30)");
    for (int v = 0; v < V; v++) {
        if (lm_idx[v] < 0 || 3 + 2 * ((long long)lm_idx[v] + 1) > d->live)
            return fail(EKF_ERR_INVALID, std::string(fnc) + ": every landmark must lie inside the live dimension");
        for (int u = 0; u < v; u++)
            if (lm_idx[u] == lm_idx[v]) return fail(EKF_ERR_INVALID, std::string(fnc) + ": the landmarks must be distinct");
    }
    const ekf::Params p = landmark_params(params);
    HIPC(hipSetDevice(d->device));
    EKFC(joint_reserve(d, fnc));
    const JointView jv = view(d->joint.p, L::joint_layout());
    const CorrSparseView cin = view(d->corr_in, L::corr_sparse_layout(d->ld));
    const int m = 2 * V, s = 3 + 2 * V;
    HIPC(hipMemcpyAsync(jv.xy, meas_xy, sizeof(double) * 2 * V, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(jv.pair_lm, lm_idx, sizeof(int) * V, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    d->finish_leave();   // (a region that is being left ends here)
    ekf::launch_dense64_joint_operands(d->x, jv.xy, jv.pair_lm, nullptr, V, p.r_meas, cin.cols, cin.Hc, cin.R, cin.nu,
                                       d->stream);
    return finish_timed(d, elapsed_ms, {{cols_out, cin.cols, sizeof(int) * s},
                                        {Hc_out, cin.Hc, sizeof(double) * m * s},
                                        {nu_out, cin.nu, sizeof(double) * m}});
}

ekf_status ekf_dense64_associate_joint(ekf_dense64_handle d, const ekf_params* params, int J, const double* meas_xy,
                                       int n_max, int* known, unsigned flags, int* assoc_out, double* best_out,
                                       int* n_groups_out, double* elapsed_ms) {
    const AssocRule r{Rule::kJoint, kJointReadings, kLmFlags, true};
    return assoc_readings_form(d, "ekf_dense64_associate_joint", r, params, J, meas_xy, n_max, known, flags, assoc_out,
                               best_out, n_groups_out, elapsed_ms);
}

// ekf_dense64_fit_scan, then the path of ekf_dense64_associate_joint on the first min(count, max_readings) centres
ekf_status ekf_dense64_associate_scan_joint(ekf_dense64_handle d, const ekf_params* params, const double* ranges,
                                            int n_beams, int max_readings, int n_max, int* known, unsigned flags,
                                            int* count_out, double* centres_out, int* assoc_out, double* best_out,
                                            double* elapsed_ms) {
    const AssocRule r{Rule::kJoint, kJointReadings, kLmFlags, true};
    return assoc_scan_form(d, "ekf_dense64_associate_scan_joint", r, params, ranges, n_beams, max_readings, n_max, known,
                           flags, count_out, centres_out, assoc_out, best_out, elapsed_ms);
}

// ---- joint compatibility: the candidates and their cross blocks on the device, the search on the host -------------------
ekf_status ekf_dense64_jcbb_launch_info(ekf_dense64_handle d, int* tile, int* threads) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_jcbb_launch_info: null handle");
    if (tile) *tile = ekf::kDense64JcbbTile;
    if (threads) *threads = ekf::kDense64JcbbTile * ekf::kDense64JcbbTile;
    return EKF_OK;
}

ekf_status ekf_dense64_jcbb_candidates(ekf_dense64_handle d, const ekf_params* params, int J, const double* meas_xy, int known,
                                       double gate_ic, int max_cand, int* cand_count_out, int* cand_lm_out,
                                       double* cand_nis_out, double* best_out, int* is_new_out, int* P_out, double* W_out,
                                       double* nu_out, double* elapsed_ms) {
    const char* fnc = "ekf_dense64_jcbb_candidates";
    const std::string fn = fnc;
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    const RegionLeave leaving(d);   // outside a region's terms: it ends behind this call's checks and e0
    if (!meas_xy) return fail(EKF_ERR_INVALID, fn + ": null argument");
    if (J < 1 || J > kJcbbReadings) return fail(EKF_ERR_INVALID, fn + ": J must lie in [1, 32]");
    if (known < 0 || known > kSparseRows / 2 || 3 + 2 * (long long)known > d->live)
        return fail(EKF_ERR_INVALID, fn + ": the known landmarks (at most 32768) must lie inside the live dimension");
    const ekf::Params p = landmark_params(params);
    EKFC(jcbb_gates_ok(fn, p, J, gate_ic, nullptr, 1));
    if (max_cand < 1 || max_cand > kJcbbCand) return fail(EKF_ERR_INVALID, fn + ": max_cand must lie in [1, 4]");
    if (!cand_count_out && !cand_lm_out && !cand_nis_out && !best_out && !is_new_out && !P_out && !W_out && !nu_out)
        return fail(EKF_ERR_INVALID, fn + ": every output is NULL");
    HIPC(hipSetDevice(d->device));
    EKFC(joint_reserve(d, fnc));
    EKFC(jcbb_reserve(d, fnc));
    const int chunk = known > 0 ? joint_chunk(J, known) : J;
    if (known > 0) EKFC(sps_reserve(d, L::sps_layout(chunk * known, 2, 5, true, false).bytes, fnc));
    const JointView jv = view(d->joint.p, L::joint_layout());
    HIPC(hipMemcpyAsync(jv.xy, meas_xy, sizeof(double) * 2 * J, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    JcbbDown down;
    EKFC(jcbb_device(d, fnc, p, jv, J, known, chunk, gate_ic, max_cand, W_out != nullptr, &down, elapsed_ms));
    const int P = down.head[0];
    for (int j = 0; j < J; j++) {
        if (cand_count_out) cand_count_out[j] = down.cand_count[j];
        if (best_out) best_out[j] = down.best[j];
        if (is_new_out) is_new_out[j] = down.is_new[j];
        for (int c = 0; c < max_cand; c++) {
            if (cand_lm_out) cand_lm_out[j * max_cand + c] = down.cand_lm[j * kJcbbCand + c];
            if (cand_nis_out) cand_nis_out[j * max_cand + c] = down.cand_nis[j * kJcbbCand + c];
        }
    }
    if (P_out) *P_out = P;
    if (nu_out) std::memcpy(nu_out, down.nu, sizeof(double) * 2 * P);
    if (W_out) jcbb_unpack_W(d->jcbb_W.data(), P, W_out);
    return EKF_OK;
}

ekf_status ekf_dense64_jcbb_search(int J, int P, const int* reading_of, const int* lm_of, const double* nis, const double* W,
                                   const double* nu, const double* gate_joint, long long max_nodes, int* assign_out,
                                   ekf_dense64_jcbb_report* report) {
    const std::string fn = "ekf_dense64_jcbb_search";
    (void)nis;   // the candidates come ranked: their scores are the caller's record, no decision reads them
    if (!gate_joint || !assign_out || (P > 0 && (!reading_of || !lm_of || !W || !nu)))
        return fail(EKF_ERR_INVALID, fn + ": null argument");
    if (ekf::jcbb_arguments_bad(J, P, reading_of, lm_of, gate_joint, max_nodes))
        return fail(EKF_ERR_INVALID, fn + ": bad argument (1 <= J <= 32, 0 <= P <= 128, reading_of ascending with at most 4 "
                                          "candidates a reading, every gate finite and > 0, 1 <= max_nodes <= 2^22)");
    ekf::JcbbSearch search(J, P, reading_of, lm_of, W, nu, gate_joint, max_nodes);
    const ekf::JcbbResult res = search.run(assign_out);
    if (report) *report = ekf_dense64_jcbb_report{P, res.n_pairs, 0, J - res.n_pairs, res.exhausted, res.nodes, res.d2};
    return EKF_OK;
}

ekf_status ekf_dense64_associate_jcbb(ekf_dense64_handle d, const ekf_params* params, int J, const double* meas_xy, int n_max,
                                      int* known, double gate_ic, const double* gate_joint, long long max_nodes,
                                      unsigned flags, int* assoc_out, double* best_out, ekf_dense64_jcbb_report* report,
                                      int* n_groups_out, double* elapsed_ms) {
    const AssocRule r{Rule::kJcbb, kJcbbReadings, kLmFlags, true, gate_ic, gate_joint, max_nodes, report};
    return assoc_readings_form(d, "ekf_dense64_associate_jcbb", r, params, J, meas_xy, n_max, known, flags, assoc_out,
                               best_out, n_groups_out, elapsed_ms);
}

// ekf_dense64_fit_scan, then the path of ekf_dense64_associate_jcbb on the first min(count, max_readings) centres
ekf_status ekf_dense64_associate_scan_jcbb(ekf_dense64_handle d, const ekf_params* params, const double* ranges, int n_beams,
                                           int max_readings, int n_max, int* known, double gate_ic, const double* gate_joint,
                                           long long max_nodes, unsigned flags, int* count_out, double* centres_out,
                                           int* assoc_out, double* best_out, ekf_dense64_jcbb_report* report,
                                           double* elapsed_ms) {
    const AssocRule r{Rule::kJcbb, kJcbbReadings, kLmFlags, true, gate_ic, gate_joint, max_nodes, report};
    return assoc_scan_form(d, "ekf_dense64_associate_scan_jcbb", r, params, ranges, n_beams, max_readings, n_max, known,
                           flags, count_out, centres_out, assoc_out, best_out, elapsed_ms);
}

// ---- the reference's prediction() and measurement() on the handle's own state ------------------------------------------
// prediction (:55-106): k_dmd_predict writes Fr, Qr and dx from state[0] where propagate_block's uploads go, then exactly
// what ekf_dense64_propagate_block(first = 0, r = 3) launches; the operands come down behind the one synchronisation.
ekf_status ekf_dense64_predict_landmarks(ekf_dense64_handle d, const ekf_params* params, double dtheta, double dx,
                                         double* Fr_out, double* dx_out, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_predict_landmarks: null handle");
    if (d->live < 3)
        return fail(EKF_ERR_INVALID, "ekf_dense64_predict_landmarks: the pose block must lie inside the live dimension");
    const ekf::Params p = landmark_params(params);
    HIPC(hipSetDevice(d->device));
    const BlkInView in = view(d->blk_in, L::blk_in_layout());
    HIPC(hipEventRecord(d->e0, d->stream));
    ekf::launch_dense64_model_predict(d->x, dtheta, dx, p.q_pose, p.straight_eps, in.Fr, in.Qr, in.dx, d->stream);
    d->carry_or_flush([&](const PendView& pv) {
        ekf::launch_dense64_panel_map(pv.K, pv.T, d->pend_rows, in.Fr, nullptr, d->ld, 0, 3, 3, d->stream);
    });
    ekf::launch_dense64_block(d->S, d->x, in.Fr, in.Qr, in.dx, d->live, d->ld, 0, 3, d->stream);
    d->region_row_map(in.Fr, nullptr, 0, 3, 3);
    return finish_timed(d, elapsed_ms, {{Fr_out, in.Fr, sizeof(double) * 9}, {dx_out, in.dx, sizeof(double) * 3}});
}

// measurement (:108-197).  [snapshot | init of all n_lm landmarks on the first call], then per visible landmark in
// ascending order [terms at the snapshot pose, wrapped | correction | heading wrap] and the correction's own
// synchronisation.  Nothing of the state comes down; the readings go up once, and only when the call initialises.
ekf_status ekf_dense64_measure_landmarks(ekf_dense64_handle d, const ekf_params* params, int n_lm, const double* sensor_xy,
                                         const uint8_t* visible, int* initialised, unsigned flags, int* corrected_out,
                                         double* Hc_out, double* nu_out, double* elapsed_ms) {
    const char* fnc = "ekf_dense64_measure_landmarks";
    const std::string fn = fnc;
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    const RegionLeave leaving((flags & EKF_DENSE64_LM_JOSEPH) ? d : nullptr);   // the Joseph form is outside a region's terms
    if (!sensor_xy || !visible || !initialised) return fail(EKF_ERR_INVALID, fn + ": null argument");
    if (n_lm < 1 || 3 + 2 * (long long)n_lm > d->live)
        return fail(EKF_ERR_INVALID, fn + ": the n_lm >= 1 landmarks must lie inside the live dimension");
    EKFC(lm_flags_ok(fn, flags, EKF_DENSE64_LM_DEFERRED | EKF_DENSE64_LM_JOSEPH));
    const bool deferred = (flags & EKF_DENSE64_LM_DEFERRED) != 0, init = *initialised == 0;
    const ekf::Params p = landmark_params(params);
    if (elapsed_ms) *elapsed_ms = 0.0;
    if (corrected_out) *corrected_out = 0;
    HIPC(hipSetDevice(d->device));
    if (deferred) EKFC(pend_reserve(d, fnc));
    const L::LmMeasureLayout l = L::lm_measure_layout(n_lm);
    EKFC(sps_reserve(d, l.bytes, fnc));
    const LmMeasureView mv = view(d->sps.p, l);
    const CorrSparseView cin = view(d->corr_in, L::corr_sparse_layout(d->ld));
    if (init) HIPC(hipMemcpyAsync(mv.xy, sensor_xy, sizeof(double) * 2 * n_lm, hipMemcpyHostToDevice, d->stream));
    LegTimer leg(elapsed_ms);
    double* pms = leg.pms();
    HIPC(hipEventRecord(d->e0, d->stream));
    d->finish_leave();   // (a region that is being left ends here)
    ekf::launch_dense64_model_snapshot(d->x, mv.pose, d->stream);                        // :109-111
    if (init) ekf::launch_dense64_model_init(mv.pose, mv.xy, n_lm, d->x, d->stream);     // :113-128, Sigma untouched
    bool open = true;   // e0 is recorded and nothing has synchronised behind it yet
    int v = 0;
    for (int i = 0; i < n_lm; i++) {
        if (!visible[i]) continue;
        if (!open) HIPC(hipEventRecord(d->e0, d->stream));
        open = false;
        // the pose of the snapshot, the landmark from the current state (get_tube_x(i)); the innovation wrapped (:183)
        ekf::launch_dense64_lm_terms(d->x, mv.pose, sensor_xy[2 * i], sensor_xy[2 * i + 1], i, 1, 1, p.r_meas, cin.cols,
                                     cin.Hc, cin.R, cin.nu, d->stream);
        correct_sparse_launch(d, deferred, 2, 5, true, lm_joseph(flags));
        ekf::launch_dense64_lm_wrap(d->x, view(d->corr_out, L::corr_out_layout()).verdict, d->stream);   // :187
        // (a refused correction's launches ran and were timed)
        const ekf_status st = leg(correct_sparse_finish(
            d, fnc, deferred, 2, nullptr, pms, {Hc_out ? Hc_out + (size_t)v * 10 : nullptr, cin.Hc, sizeof(double) * 10},
            {nu_out ? nu_out + (size_t)v * 2 : nullptr, cin.nu, sizeof(double) * 2}));
        if (init && (st == EKF_OK || st == EKF_ERR_STATE)) *initialised = 1;   // the initialisation has completed and stands
        if (st != EKF_OK) return st;
        v++;
        if (corrected_out) *corrected_out = v;
    }
    if (open) {   // nothing visible: the snapshot (and the initialisation) alone
        EKFC(leg(finish_timed(d, pms)));
        if (init) *initialised = 1;
    }
    return EKF_OK;
}

}  // extern "C"
