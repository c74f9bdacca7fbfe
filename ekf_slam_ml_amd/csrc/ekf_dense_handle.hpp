// ekf_dense_handle.hpp -- the two dense handles behind include/ekfslam.h, shared by ekf_capi_dense.hip (the fp32 entry
// points and the templates over the element type) and ekf_capi_dense64.hip (everything only the fp64 handle has).  The
// templates reach what is particular to a handle through four hooks -- created, destroying, sigma_needed, sigma_replaced --
// which are empty for fp32.  Every device buffer of a handle, at creation or later (DeviceBuf), comes from the handle's
// ledger (ekf_device_mem.hpp).  Also here: the typed views of the
// layouts of ekf_dense64_layout.hpp, and the end of a timed entry point.
#pragma once
#include "ekf_dense64_region_mem.hpp"
#include "ekf_runtime.hpp"

namespace ekfrt {

template <class E>
struct DenseHandle {
    int device = -1, N = 0, ld = 0;
    hipStream_t stream = nullptr;
    Ledger mem;   // every device allocation of the handle
    E *F = nullptr, *S = nullptr, *T = nullptr, *Q = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // the hooks of the shared templates; a handle with more than Sigma hides them with its own
    ekf_status created() { return EKF_OK; }   // inside create, stream and Sigma exist: the handle's own buffers
    void destroying() {}                      // inside destroy, the ledger is empty: what else the handle holds
    void sigma_needed() {}                    // Sigma is about to be read or written in memory, inside the timed region
    void sigma_replaced() {}                  // set() gave a new Sigma
};

// ---- typed views of the fp64 handle's operand buffers: a base pointer and a layout ---------------------------------------
inline double* f64(void* base, size_t off) { return reinterpret_cast<double*>(static_cast<char*>(base) + off); }
inline int* i32(void* base, size_t off) { return reinterpret_cast<int*>(static_cast<char*>(base) + off); }
namespace L = ekf::d64;
struct CorrInView { double *H, *Ht, *R, *nu; };
inline CorrInView view(void* b, const L::CorrInLayout& l) { return {f64(b, l.H), f64(b, l.Ht), f64(b, l.R), f64(b, l.nu)}; }
struct CorrSparseView { double* Hc; int* cols; double *R, *nu; };
inline CorrSparseView view(void* b, const L::CorrSparseLayout& l) { return {f64(b, l.Hc), i32(b, l.cols), f64(b, l.R), f64(b, l.nu)}; }
struct CorrOutView { double* nis; int* verdict; unsigned long long* words; };   // words: the coupling's two, on the same 16 bytes
inline CorrOutView view(void* b, const L::CorrOutLayout& l) {
    return {f64(b, l.nis), i32(b, l.verdict), reinterpret_cast<unsigned long long*>(f64(b, l.nis))};
}
struct ScSmallView { double *R, *nu, *nis, *S; int* flag; };
inline ScSmallView view(void* b, const L::ScSmallLayout& l) { return {f64(b, l.R), f64(b, l.nu), f64(b, l.nis), f64(b, l.S), i32(b, l.flag)}; }
struct BlkInView { double *Fr, *Qr, *dx; };
inline BlkInView view(void* b, const L::BlkInLayout& l) { return {f64(b, l.Fr), f64(b, l.Qr), f64(b, l.dx)}; }
struct IniInView { double *G, *W, *xb; int* cols; };
inline IniInView view(void* b, const L::IniInLayout& l) { return {f64(b, l.G), f64(b, l.W), f64(b, l.xb), i32(b, l.cols)}; }
struct RdBufView { double* out; int *rows, *cols; };
inline RdBufView view(void* b, const L::RdBufLayout& l) { return {f64(b, l.out), i32(b, l.rows), i32(b, l.cols)}; }
struct PendView { double *K, *T; const int* zero; };   // all null before the first deferred call
inline PendView view(void* b, const L::PendLayout& l) {
    return b ? PendView{f64(b, l.K), f64(b, l.T), i32(b, l.zero)} : PendView{nullptr, nullptr, nullptr};
}
struct SpsView { double *Hc, *R, *nu, *nis, *S; int *cols, *flag; };   // S null unless asked for
inline SpsView view(void* b, const L::SpsLayout& l, bool want_S) {
    return {f64(b, l.Hc), f64(b, l.R), f64(b, l.nu), f64(b, l.nis), want_S ? f64(b, l.S) : nullptr, i32(b, l.cols), i32(b, l.flag)};
}
struct LmMeasureView { double *pose, *xy; };
inline LmMeasureView view(void* b, const L::LmMeasureLayout& l) { return {f64(b, l.pose), f64(b, l.xy)}; }
struct ScanView { double* ranges; int* head; double *centres, *radii, *all; };
inline ScanView view(void* b, const L::ScanLayout& l) { return {f64(b, l.ranges), i32(b, l.head), f64(b, l.centres), f64(b, l.radii), f64(b, l.all)}; }
struct JointView { double* xy; ekf::Dense64LmRecord* pre; int* head; ekf::Dense64LmRecord* rec; double* xb; int *pair_lm, *pair_j; double *W_full, *W_last; };
inline JointView view(void* b, const L::JointLayout& l) {
    return {f64(b, l.xy), reinterpret_cast<ekf::Dense64LmRecord*>(f64(b, l.pre)), i32(b, l.head),
            reinterpret_cast<ekf::Dense64LmRecord*>(f64(b, l.rec)), f64(b, l.xb), i32(b, l.pair_lm), i32(b, l.pair_j),
            f64(b, l.W_full), f64(b, l.W_last)};
}
struct JcbbView { int *head, *cand_count, *offset, *is_new, *cand_lm, *reading_of, *lm_of; double *best, *cand_nis, *nu; int* cols; double *Hc, *W; };
inline JcbbView view(void* b, const L::JcbbLayout& l) {
    return {i32(b, l.head), i32(b, l.cand_count), i32(b, l.offset), i32(b, l.is_new), i32(b, l.cand_lm), i32(b, l.reading_of),
            i32(b, l.lm_of), f64(b, l.best), f64(b, l.cand_nis), f64(b, l.nu), i32(b, l.cols), f64(b, l.Hc), f64(b, l.W)};
}

// The end of a timed entry point: e1 behind the launches, the launch error, the copies back to the host (a null dst is
// skipped), ONE synchronisation, the time between the handle's events.
struct CopyBack { void* dst; const void* src; size_t bytes; };
template <class H>
ekf_status finish_timed(H* d, double* elapsed_ms, std::initializer_list<CopyBack> back = {}) {
    HIPC(hipEventRecord(d->e1, d->stream));
    HIPC(hipGetLastError());
    for (const CopyBack& c : back)
        if (c.dst) HIPC(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    if (elapsed_ms) {
        float ms = 0.f;
        HIPC(hipEventElapsedTime(&ms, d->e0, d->e1));
        *elapsed_ms = ms;
    }
    return EKF_OK;
}

}  // namespace ekfrt

struct ekf_dense_s : ekfrt::DenseHandle<float> {};

struct ekf_dense64_s : ekfrt::DenseHandle<double> {
    // allocated with the handle (created): the state vector, and the operands of the calls whose sizes are fixed
    double* x = nullptr;         // [ld], zero beyond N
    double* corr_in = nullptr;   // CorrInLayout (ekf_dense64_correct) or CorrSparseLayout (the sparse corrections)
    double* corr_out = nullptr;  // CorrOutLayout
    double* ws_own = nullptr;    // workspace of a handle too small for it to fit the product buffer T
    double* blk_in = nullptr;    // BlkInLayout (ekf_dense64_propagate_block)
    double* ini_in = nullptr;    // IniInLayout (ekf_dense64_init_block, the landmark front end)
    double* rd_buf = nullptr;    // RdBufLayout (ekf_dense64_get_sigma_block)
    // nothing until the first call that needs them; sc_H, sc_ws and sps grow with the calls
    ekfrt::DeviceBuf sc_small;   // ScSmallLayout (ekf_dense64_score)
    ekfrt::DeviceBuf sc_H;       // the stacked Jacobians, [groups * 64][ld], columns N .. ld zero
    ekfrt::DeviceBuf sc_ws;      // the partial S blocks of a call that do not fit the product buffer T
    ekfrt::DeviceBuf sps;        // SpsLayout (ekf_dense64_score_sparse, the landmark front end), cut per call; LmMeasureLayout
    ekfrt::DeviceBuf pend;       // PendLayout (ekf_dense64_correct_sparse_deferred)
    ekfrt::DeviceBuf lm_rec;     // ekf::Dense64LmRecord, the decision record of one reading (the landmark front end)
    ekfrt::DeviceBuf scan;       // ScanLayout (ekf_dense64_fit_scan, ekf_dense64_associate_scan)
    ekfrt::DeviceBuf joint;      // JointLayout (ekf_dense64_associate_joint, ekf_dense64_joint_operands)
    ekfrt::DeviceBuf jcbb;       // JcbbLayout (ekf_dense64_jcbb_candidates, ekf_dense64_associate_jcbb), reserved once for its maxima
    ekfrt::DeviceBuf pairs;      // Dense64PairsPlan (ekf_dense64_score_landmark_pairs), grows with n_lm
    ekfrt::DeviceBuf health;     // Dense64HealthPlan (ekf_dense64_health, ekf_dense64_symmetrize), grows with live
    ekfrt::DeviceBuf value;      // Dense64ValuePlan (ekf_dense64_value_operands, ekf_dense64_rank_landmarks), grows with count and live
    ekfrt::DeviceBuf factor;     // the snapshot of ekf_dense64_factor: L of the live corner, Dense64FactorPlan::factor_bytes
    ekfrt::DeviceBuf factor_ws;  // Dense64FactorPlan: the verdict word, the per-block records, the diagonal of L
    ekfrt::DeviceBuf whiten;     // ekf_dense64_whiten: the working copy of B and Y, then d2
    ekfrt::DeviceBuf frame;      // Dense64FramePlan (ekf_dense64_map_congruence, ekf_dense64_reframe_landmarks), a function of ld
    ekfrt::DeviceBuf join;       // Dense64JoinPlan (ekf_dense64_join_congruence, ekf_dense64_join_map) of the DESTINATION, grows with Nb
    ekfrt::DeviceBuf extract;    // Dense64ExtractPlan (ekf_dense64_extract_map) of the DESTINATION: the list and the run flags, grows with k
    ekfrt::DeviceBuf evidence;   // Dense64EvidencePlan (ekf_dense64_scan_evidence), grows with count
    ekfrt::StagingRing scan_up;  // pinned: a scan's ranges on their way up, reserved with `scan` or `evidence`
    std::vector<double> scan_rec; // the record of a scan as it came down (ScanLayout from head on)
    std::vector<double> host_in; // the dense correction's operands, packed for their three uploads
    std::vector<int> host_stamp; // [N] the duplicate check of the index lists
    std::vector<double> jcbb_W;  // the cross blocks of a joint compatibility call as they came down, [P][P][2][2]
    std::vector<int> host_keep;  // ekf_dense64_extract_map: the list and the run flags on their way up
    int pend_rows = 0;           // rows of the two panels that wait for the flush, 0 .. 64
    int factor_na = 0;           // the live dimension the snapshot was taken at, 0 before the first factor
    int factor_ok = 0;           // the snapshot is a complete factor (the last ekf_dense64_factor ended with ok == 1)
    int carry = 0;               // ekf_dense64_set_carry: propagate_block, init_block, swap_blocks, get_sigma_block do not flush
    // the live dimension (ekf_dense64_set_live): what the structured calls take for N; the plans change with it, not per call
    int live = 0;                          // 1 .. N, N unless set
    ekf::Dense64CorrectPlan pl_full{};     // of (N, ld): the dense correction, and the layout of the workspace
    ekf::Dense64CorrectPlan pl_live{};     // of (live, ld) on that layout: the sparse corrections and the flush

    // a local region (ekf_dense64_region_begin): the accumulators and the scratch of the global update, one group of the
    // ledger that stays for the next region of the same size; the live value to go back to; what the region absorbed
    ekfrt::RegionMem region_mem;           // the accumulators and the scratch (ekf_dense64_region_mem.hpp)
    int region_on = 0;                     // a region is open
    int region_back = 0;                   // the live dimension region_end restores
    long long region_corrections = 0, region_row_maps = 0;   // of the open region, or of the last one
    long long region_ended_by_other = 0;   // regions of this handle that a call outside the region's terms ended
    ekf::Dense64RegionPlan region_pl{};
    int region_leaving = 0;                // a call outside the terms is between its checks and its first launch (begin_leave)

    ekf_status created();
    void destroying();
    void sigma_needed() { begin_leave(); flush_pending(); }   // (the flush ends a region that is being left)
    void sigma_replaced() { pend_rows = 0; }   // the pending rows belonged to the covariance that was replaced

    double* workspace() const { return ws_own ? ws_own : T; }   // (the product buffer is dead between propagations)
    // ---- the pending rows: K and T of the deferred corrections, Sigma_cur = Sigma - K^T T ---------------------------------
    ekfrt::PendView panels() const { return ekfrt::view(pend.p, ekf::d64::pend_layout(ld)); }
    bool carries() const { return carry && pend_rows > 0; }   // this call leaves the rows pending and works through them
    // Sigma <- Sigma_cur: one launch on the handle's stream when rows are pending, nothing otherwise.  For every entry point
    // that reads or writes Sigma in memory, after its argument checks and inside its timed region.
    void flush_pending() {
        finish_leave();   // a call outside a region's terms: the region ends here, behind the call's e0
        if (pend_rows == 0) return;
        const ekfrt::PendView p = panels();
        ekf::launch_dense64_flush(pl_live, S, p.K, p.T, pend_rows, p.zero, stream);
        pend_rows = 0;
    }
    // A call that is a congruence on Sigma: the rows take it too (the caller's launch on the panels) when the handle carries
    // them, and are applied first otherwise.
    template <class Launch>
    void carry_or_flush(Launch&& on_panels) {
        finish_leave();
        if (carries()) on_panels(panels());
        else flush_pending();
    }
    // ---- the local region ----------------------------------------------------------------------------------------------
    // The end of a region, launches only, on the handle's stream: the pending rows at width Na, the global update, the live
    // dimension the region found.  (The accumulators are set again by the next region_begin.)
    void close_region() {
        flush_pending();
        if (region_corrections || region_row_maps)   // (a region that absorbed nothing owes nothing: every bit stays)
            ekf::launch_dense64_region_end(region_pl, S, x, region_mem.acc, region_mem.scratch, stream);
        region_on = 0;
        live = region_back;
        pl_live = ekf::dense64_live_plan(pl_full, live);
    }
    // An entry point outside the region's terms leaves in two steps, so that a refused call ends nothing and the global
    // update runs inside the call's own timed region.  begin_leave (through RegionLeave, on entry): host only -- the live
    // dimension the region found is back, so the call checks its arguments as it always did.  finish_leave (behind the call's
    // e0: inside flush_pending and carry_or_flush, or spelled where a call has neither): the launches.  cancel_leave
    // (RegionLeave's destructor): the call returned before its first launch, the region stays open.
    void begin_leave() {
        if (!region_on || region_leaving) return;
        region_leaving = 1;
        live = region_back;
        pl_live = ekf::dense64_live_plan(pl_full, live);
    }
    void finish_leave() {
        if (!region_leaving) return;
        region_leaving = 0;
        live = region_pl.Na;   // (the pending rows have the region's width)
        pl_live = ekf::dense64_live_plan(pl_full, live);
        (void)hipSetDevice(device);
        close_region();
        region_ended_by_other++;
    }
    void cancel_leave() {
        if (!region_leaving) return;
        region_leaving = 0;
        live = region_pl.Na;
        pl_live = ekf::dense64_live_plan(pl_full, live);
    }
    // the two steps at once: for the calls that have no timed region and check nothing against the live dimension
    void leave_region() {
        begin_leave();
        finish_leave();
    }
    // the accumulator step of a call inside a region, behind the live call's own launches
    void region_row_map(const double* M, const int* src, int first, int r, int s) {
        if (!region_on) return;
        ekf::launch_dense64_region_rowmap(region_pl, region_mem.acc, M, src, first, r, s, stream);
        region_row_maps++;
    }
};

// on entry of a call outside a region's terms (d may be null: nothing)
struct RegionLeave {
    ekf_dense64_s* d;
    explicit RegionLeave(ekf_dense64_s* h) : d(h) { if (d) d->begin_leave(); }
    ~RegionLeave() { if (d) d->cancel_leave(); }
    RegionLeave(const RegionLeave&) = delete;
    RegionLeave& operator=(const RegionLeave&) = delete;
};
