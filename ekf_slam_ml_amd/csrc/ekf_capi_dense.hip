// ekf_capi_dense.hip -- C ABI of include/ekfslam.h, dense general-F covariance propagation: fp32 MFMA (configs[3],
// ekf_dense.hip) and its fp64 twin (ekf_dense64.hip).  The host side of the two handles is one template over the element
// type; the kernels stay separate.  The fp64 handle also owns a state vector, the dense measurement update for a
// general Jacobian (ekf_dense64_correct.hip), the read-only scoring of candidate measurements (ekf_dense64_score.hip),
// the block-structured prediction (ekf_dense64_block.hip), the update and scoring for a Jacobian given by its non-zero
// columns (ekf_dense64_sparse.hip), the (re)initialisation of a block of states and the block readout
// (ekf_dense64_init.hip), the exchange of two blocks of states (ekf_dense64_swap.hip), and the deferred form of the sparse
// update (the second instantiation of ekf_dense64_sparse.hip's kernels): pending rows of K and T that the sparse calls read through and every other call that touches Sigma applies
// first (flush_pending) -- unless the caller lets propagate_block, init_block, swap_blocks and the block readout carry them
// (ekf_dense64_set_carry, ekf_dense64_carry.hip).  The structured calls run at the handle's LIVE dimension
// (ekf_dense64_set_live, N by default): every launch of theirs is cut for it, and nothing at an index from it on is read
// or written; ekf_dense64_coupling (ekf_dense64_live.hip) measures what ties the live corner to the rest.
#include "ekf_runtime.hpp"

#include <type_traits>

using namespace ekfrt;

template <class E>
struct DenseHandle {
    int device = -1, N = 0, ld = 0;
    hipStream_t stream = nullptr;
    E *F = nullptr, *S = nullptr, *T = nullptr, *Q = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
};
struct ekf_dense_s : DenseHandle<float> {};
struct ekf_dense64_s : DenseHandle<double> {
    // measurement update (ekf_dense64_correct): the state vector, the operands of one correction, its verdict and score
    double* x = nullptr;        // [ld], zero beyond N
    double* corr_in = nullptr;  // H [64][ld] | H^T [ld][m rounded up to 16] (room for 64) | R [64 * 64] | nu [64]
    double* corr_out = nullptr; // nis | verdict (an int in the second double)
    double* ws_own = nullptr;   // workspace of a handle too small for it to fit the product buffer T
    std::vector<double> host_in;
    // candidate scoring (ekf_dense64_score): nothing until the first call; the two large buffers grow with the calls
    double* sc_small = nullptr;  // R [2048 * 64] | nu [2048] | nis [2048] | S [2048 * 64] | flags (ints) [2048]
    double* sc_H = nullptr;      // the stacked Jacobians, [groups * 64][ld], columns N .. ld zero
    double* sc_ws = nullptr;     // the partial S blocks of a call that do not fit the product buffer T
    size_t sc_H_doubles = 0, sc_ws_doubles = 0;
    // block-structured prediction (ekf_dense64_propagate_block)
    double* blk_in = nullptr;    // Fr [64 * 64] | Qr [64 * 64] | dx [64]
    // column-sparse scoring (ekf_dense64_score_sparse): one buffer, nothing until the first call, grows with the calls
    char* sps = nullptr;         // Hc | R | nu | nis | S | cols (ints) | flags (ints), cut per call
    size_t sps_bytes = 0;
    std::vector<int> host_stamp; // [N] the duplicate check of the index lists
    // (re)initialisation of a block (ekf_dense64_init_block) and the block readout (ekf_dense64_get_sigma_block)
    double* ini_in = nullptr;    // G [64 * 64] | W [64 * 64] | xb [64] | cols (ints) [64]
    double* rd_buf = nullptr;    // out [65536] | rows (ints) [65536] | cols (ints) [65536]
    // deferred sparse corrections (ekf_dense64_correct_sparse_deferred): nothing until the first call
    double* pend = nullptr;      // K^T [64][ld] | T [64][ld] | a word kept at zero (the flush's verdict argument)
    int pend_rows = 0;           // rows of the two panels that wait for the flush, 0 .. 64
    int carry = 0;               // ekf_dense64_set_carry: propagate_block, init_block, get_sigma_block do not flush
    // the live dimension (ekf_dense64_set_live): what the structured calls take for N; the plans change with it, not per call
    int live = 0;                          // 1 .. N, N unless set
    ekf::Dense64CorrectPlan pl_full{};     // of (N, ld): the dense correction, and the layout of the workspace
    ekf::Dense64CorrectPlan pl_live{};     // of (live, ld) on that layout: the sparse corrections and the flush
    // the landmark front end (ekf_dense64_associate_landmarks): nothing until the first call
    ekf::Dense64LmRecord* lm_rec = nullptr;   // the decision record of one reading
};

namespace {

// per element type: the launcher, the split report and the LDS-limit set-up of ekf_dense.hpp
struct DenseOps32 {
    static hipError_t prepare() { return ekf::dense_gemm_prepare(); }
    static void gemm(const float* A, const float* B, float* C, const float* Qadd, int ld, bool bt, hipStream_t s, int n) {
        ekf::launch_dense_gemm(A, B, C, Qadd, ld, bt, s, n);
    }
    static void split(int ld, int* tiles, int* n_big, int* n_tail) { ekf::dense_gemm_split(ld, tiles, n_big, n_tail); }
    static void tile_map(int ld, unsigned char* map) { ekf::dense_gemm_tile_map(ld, map); }
};
struct DenseOps64 {
    static hipError_t prepare() { return ekf::dense64_gemm_prepare(); }
    static void gemm(const double* A, const double* B, double* C, const double* Qadd, int ld, bool bt, hipStream_t s,
                     int n) {
        ekf::launch_dense64_gemm(A, B, C, Qadd, ld, bt, s, n);
    }
    static void split(int ld, int* tiles, int* n_big, int* n_tail) { ekf::dense64_gemm_split(ld, tiles, n_big, n_tail); }
    static void tile_map(int ld, unsigned char* map) { ekf::dense64_gemm_tile_map(ld, map); }
};

constexpr int kMaxM = ekf::kDense64MaxM;
constexpr int kMaxR = ekf::kDense64MaxR;
constexpr size_t kBlkQ = (size_t)kMaxR * kMaxR, kBlkDx = 2 * kBlkQ, kBlkIn = kBlkDx + kMaxR;
constexpr size_t kIniW = (size_t)kMaxR * ekf::kDense64MaxS, kIniXb = kIniW + (size_t)kMaxR * kMaxR, kIniCols = kIniXb + kMaxR,
                 kIniIn = kIniCols + ekf::kDense64MaxS / 2;
constexpr int kReadMax = ekf::kDense64ReadMax;
constexpr size_t kRdRows = kReadMax, kRdCols = kRdRows + kReadMax / 2, kRdBuf = kRdCols + kReadMax / 2;
inline size_t corr_in_doubles(int ld) { return (size_t)2 * kMaxM * ld + kMaxM * kMaxM + kMaxM; }
constexpr int kMaxP = ekf::kDense64PendingMaxRows;
inline size_t pend_T(int ld) { return (size_t)kMaxP * ld; }
inline size_t pend_zero(int ld) { return 2 * pend_T(ld); }

// Sigma <- Sigma_cur: one launch on the handle's stream when rows are pending, nothing otherwise.  Called by every entry
// point that reads or writes Sigma in memory, after its argument checks and inside its timed region.
template <class H>
void flush_pending(H* d) {
    if constexpr (std::is_same<H, ekf_dense64_s>::value) {
        if (d->pend_rows == 0) return;
        ekf::launch_dense64_flush(d->pl_live, d->S, d->pend, d->pend + pend_T(d->ld), d->pend_rows, reinterpret_cast<const int*>(d->pend + pend_zero(d->ld)), d->stream);
        d->pend_rows = 0;
    }
}

// The pending rows through a congruence with A = identity except rows [first, first + r) (ekf_dense64_carry.hip): mapped
// when the handle carries them, applied to Sigma otherwise.  M, src: the operands the entry point has already sent up.
void carry_or_flush(ekf_dense64_s* d, const double* M, const int* src, int first, int r, int s) {
    if (d->carry && d->pend_rows > 0)
        ekf::launch_dense64_panel_map(d->pend, d->pend + pend_T(d->ld), d->pend_rows, M, src, d->ld, first, r, s,
                                      d->stream);
    else
        flush_pending(d);
}

// The end of a timed entry point: e1 behind the launches, the launch error, the copies back to the host (a null dst is
// skipped), ONE synchronisation, the time between the handle's events.
struct CopyBack {
    void* dst;
    const void* src;
    size_t bytes;
};
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

// finish_timed of a correction: corr_out (nis | verdict) comes back in one copy; *verdict: 0 = applied, 1 = S singular.
ekf_status finish_correction(ekf_dense64_s* d, double* elapsed_ms, double* nis, int* verdict) {
    double out[2] = {0.0, 0.0};
    EKFC(finish_timed(d, elapsed_ms, {{out, d->corr_out, sizeof(out)}}));
    *nis = out[0];
    std::memcpy(verdict, &out[1], sizeof(int));
    return EKF_OK;
}

template <class H>
ekf_status dense_destroy(H* d) {
    if (!d) return EKF_OK;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    if (d->stream) (void)hipStreamSynchronize(d->stream);
    for (auto* p : {d->F, d->S, d->T, d->Q})
        if (p) (void)hipFree(p);
    if constexpr (std::is_same<H, ekf_dense64_s>::value)
        for (double* p : {d->x, d->corr_in, d->corr_out, d->ws_own, d->sc_small, d->sc_H, d->sc_ws, d->blk_in, d->ini_in,
                          d->rd_buf, d->pend})
            if (p) (void)hipFree(p);
    if constexpr (std::is_same<H, ekf_dense64_s>::value)
        if (d->sps) (void)hipFree(d->sps);
    if constexpr (std::is_same<H, ekf_dense64_s>::value)
        if (d->lm_rec) (void)hipFree(d->lm_rec);
    for (hipEvent_t e : {d->e0, d->e1})
        if (e) (void)hipEventDestroy(e);
    if (d->stream) (void)hipStreamDestroy(d->stream);
    delete d;
    return EKF_OK;
}

template <class H, class Ops>
ekf_status dense_create(const char* name, int N, int device, H** out) {
    if (!out || N <= 0) return fail(EKF_ERR_INVALID, std::string(name) + ": bad argument");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(EKF_ERR_NO_DEVICE, "no HIP device visible: libekfslam_hip has no CPU path");
    if (device < 0) HIPC(hipGetDevice(&device));
    if (device >= count) return fail(EKF_ERR_INVALID, "device index out of range");
    hipDeviceProp_t prop;
    HIPC(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(EKF_ERR_NO_DEVICE, std::string("kernels are built for gfx950 only, device is ") + prop.gcnArchName);
    H* d = new (std::nothrow) H();
    if (!d) return fail(EKF_ERR_NOMEM, "host allocation failed");
    d->device = device;
    d->N = N;
    d->ld = round_up(N, ekf::kDenseTile);
    const size_t bytes = sizeof(*d->F) * (size_t)d->ld * d->ld;
    ekf_status st = EKF_OK;
    auto body = [&]() -> ekf_status {
        HIPC(hipSetDevice(device));
        HIPC(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        HIPC(Ops::prepare());
        for (auto** p : {&d->F, &d->S, &d->T, &d->Q}) {
            HIPC(hipMalloc((void**)p, bytes));
            HIPC(hipMemsetAsync(*p, 0, bytes, d->stream));
        }
        if constexpr (std::is_same<H, ekf_dense64_s>::value) {
            HIPC(ekf::dense64_correct_prepare());
            const size_t in = sizeof(double) * corr_in_doubles(d->ld);
            HIPC(hipMalloc((void**)&d->x, sizeof(double) * d->ld));
            HIPC(hipMemsetAsync(d->x, 0, sizeof(double) * d->ld, d->stream));
            HIPC(hipMalloc((void**)&d->corr_in, in));
            HIPC(hipMemsetAsync(d->corr_in, 0, in, d->stream));
            HIPC(hipMalloc((void**)&d->corr_out, 2 * sizeof(double)));
            d->live = N;
            d->pl_full = d->pl_live = ekf::dense64_correct_plan(N, d->ld);
            const size_t ws = d->pl_full.ws_doubles;
            if (ws > (size_t)d->ld * d->ld) HIPC(hipMalloc((void**)&d->ws_own, sizeof(double) * ws));
            HIPC(ekf::dense64_block_prepare());
            HIPC(hipMalloc((void**)&d->blk_in, sizeof(double) * kBlkIn));
            HIPC(ekf::dense64_sparse_prepare());
            HIPC(ekf::dense64_init_prepare());
            HIPC(hipMalloc((void**)&d->ini_in, sizeof(double) * kIniIn));
            HIPC(hipMalloc((void**)&d->rd_buf, sizeof(double) * kRdBuf));
        }
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
    if constexpr (std::is_same<H, ekf_dense64_s>::value)
        if (Sigma) d->pend_rows = 0;   // the pending rows belonged to the covariance that was replaced
    return EKF_OK;
}

template <class Ops, class H>
ekf_status dense_propagate(const char* name, H* d, int iterations, double* elapsed_ms) {
    if (!d || iterations < 0) return fail(EKF_ERR_INVALID, std::string(name) + ": bad argument");
    HIPC(hipSetDevice(d->device));
    HIPC(hipEventRecord(d->e0, d->stream));
    flush_pending(d);
    for (int it = 0; it < iterations; it++) {
        Ops::gemm(d->F, d->S, d->T, nullptr, d->ld, false, d->stream, d->N);  // T = At*sigma (:102)
        Ops::gemm(d->T, d->F, d->S, d->Q, d->ld, true, d->stream, d->N);      // sigma = T*At.t() + Q
    }
    return finish_timed(d, elapsed_ms);
}

template <class Ops, class H>
ekf_status dense_launch_info(H* d, int* ld, int* tiles, int* n_big, int* n_tail) {
    if (!d) return fail(EKF_ERR_INVALID, "null handle");
    if (ld) *ld = d->ld;
    Ops::split(d->ld, tiles, n_big, n_tail);
    return EKF_OK;
}

template <class Ops, class H>
ekf_status dense_tile_map(H* d, unsigned char* map) {
    if (!d || !map) return fail(EKF_ERR_INVALID, "null argument");
    Ops::tile_map(d->ld, map);
    return EKF_OK;
}

template <class H, class E>
ekf_status dense_get_sigma(H* d, E* out) {
    if (!d || !out) return fail(EKF_ERR_INVALID, "null argument");
    HIPC(hipSetDevice(d->device));
    flush_pending(d);
    const size_t w = sizeof(E) * d->N, pitch = sizeof(E) * d->ld;
    HIPC(hipMemcpy2DAsync(out, w, d->S, pitch, w, d->N, hipMemcpyDeviceToHost, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}

// One correction: the operands go up (H twice: as given, zero padded to ld, and transposed with m rounded up to 16), the six
// launches are timed by the handle's events, the verdict and nis come back in one copy.
ekf_status dense64_correct(ekf_dense64_s* d, int m, const double* H, const double* R, const double* nu, double* nis_out,
                           double* elapsed_ms) {
    if (!d || !H || !R || m < 1 || m > kMaxM || m > d->N || (nis_out && !nu))
        return fail(EKF_ERR_INVALID, "ekf_dense64_correct: bad argument");
    HIPC(hipSetDevice(d->device));
    const int N = d->N, ld = d->ld;
    const size_t oHt = (size_t)kMaxM * ld, oR = 2 * oHt, oNu = oR + kMaxM * kMaxM;
    const int mp = round_up(m, 16);   // row length of the transposed copy
    d->host_in.assign(corr_in_doubles(ld), 0.0);
    double* in = d->host_in.data();
    for (int k = 0; k < m; k++)
        for (int j = 0; j < N; j++) {
            const double v = H[(size_t)k * N + j];
            in[(size_t)k * ld + j] = v;
            in[oHt + (size_t)j * mp + k] = v;
        }
    std::memcpy(in + oR, R, sizeof(double) * m * m);
    if (nu) std::memcpy(in + oNu, nu, sizeof(double) * m);
    const size_t piece[3][2] = {{0, (size_t)m * ld}, {oHt, (size_t)ld * mp}, {oR, (size_t)kMaxM * kMaxM + kMaxM}};
    for (const auto& pc : piece)
        HIPC(hipMemcpyAsync(d->corr_in + pc[0], in + pc[0], sizeof(double) * pc[1], hipMemcpyHostToDevice, d->stream));
    const ekf::Dense64CorrectPlan& pl = d->pl_full;
    double* ws = d->ws_own ? d->ws_own : d->T;   // (the product buffer is dead between propagations)
    HIPC(hipEventRecord(d->e0, d->stream));
    flush_pending(d);
    ekf::launch_dense64_correct(pl, d->S, d->x, ws, d->corr_in, d->corr_in + oHt, d->corr_in + oR,
                                nu ? d->corr_in + oNu : nullptr, m, d->corr_out, reinterpret_cast<int*>(d->corr_out + 1),
                                d->stream);
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
constexpr int kScoreRows = ekf::kDense64ScoreMaxRows;
constexpr size_t kScR = 0, kScNu = (size_t)kScoreRows * kMaxM, kScNis = kScNu + kScoreRows, kScS = kScNis + kScoreRows,
                 kScFlag = kScS + (size_t)kScoreRows * kMaxM, kScSmall = kScFlag + kScoreRows / 2;

// Buffers of the first / a larger call: allocated into locals, the members change only when everything succeeded.
ekf_status score_reserve(ekf_dense64_s* d, const ekf::Dense64ScorePlan& sp) {
    const bool own_ws = sp.spart_doubles > (size_t)d->ld * d->ld;   // else the product buffer, dead between propagations
    double *small = nullptr, *Hs = nullptr, *ws = nullptr;
    hipError_t e = hipSuccess;
    if (!d->sc_small) {
        e = ekf::dense64_score_prepare();
        if (e == hipSuccess) e = hipMalloc((void**)&small, sizeof(double) * kScSmall);
    }
    if (e == hipSuccess && sp.h_doubles > d->sc_H_doubles) {
        e = hipMalloc((void**)&Hs, sizeof(double) * sp.h_doubles);
        if (e == hipSuccess) e = hipMemsetAsync(Hs, 0, sizeof(double) * sp.h_doubles, d->stream);
    }
    if (e == hipSuccess && own_ws && sp.spart_doubles > d->sc_ws_doubles)
        e = hipMalloc((void**)&ws, sizeof(double) * sp.spart_doubles);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(d->stream);
        for (double* p : {small, Hs, ws})
            if (p) (void)hipFree(p);
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? EKF_ERR_NOMEM : EKF_ERR_HIP,
                    std::string("ekf_dense64_score: ") + hipGetErrorString(e) + " while reserving the candidates' buffers");
    }
    if (small) d->sc_small = small;
    if (Hs) {
        if (d->sc_H) (void)hipFree(d->sc_H);   // (synchronises; no scoring call is in flight)
        d->sc_H = Hs;
        d->sc_H_doubles = sp.h_doubles;
    }
    if (ws) {
        if (d->sc_ws) (void)hipFree(d->sc_ws);
        d->sc_ws = ws;
        d->sc_ws_doubles = sp.spart_doubles;
    }
    return EKF_OK;
}

ekf_status dense64_score(ekf_dense64_s* d, int J, int m, const double* H, const double* R, int r_shared,
                         const double* nu, double* nis_out, double* S_out, int* flag_out, double* elapsed_ms) {
    if (!d || !H || !R || J < 1 || m < 1 || m > kMaxM || m > d->N || (long long)J * m > kScoreRows ||
        (nis_out && !nu) || (!nis_out && !S_out && !flag_out))
        return fail(EKF_ERR_INVALID, "ekf_dense64_score: bad argument");
    HIPC(hipSetDevice(d->device));
    const int N = d->N, ld = d->ld;
    const ekf::Dense64ScorePlan sp = ekf::dense64_score_plan(N, ld, J, m);
    const ekf_status st = score_reserve(d, sp);
    if (st != EKF_OK) return st;
    const size_t mm = (size_t)m * m, w = sizeof(double) * N;
    const int per = sp.cpg * m;   // rows of a full group
    if (per == ekf::kDense64ScoreGroup) {
        HIPC(hipMemcpy2DAsync(d->sc_H, sizeof(double) * ld, H, w, w, (size_t)J * m, hipMemcpyHostToDevice, d->stream));
    } else {
        for (int g = 0; g < sp.n_groups; g++) {
            const int rows = std::min(sp.cpg, J - g * sp.cpg) * m;
            HIPC(hipMemcpy2DAsync(d->sc_H + (size_t)g * ekf::kDense64ScoreGroup * ld, sizeof(double) * ld,
                                  H + (size_t)g * per * N, w, w, rows, hipMemcpyHostToDevice, d->stream));
        }
    }
    double* sm = d->sc_small;
    HIPC(hipMemcpyAsync(sm + kScR, R, sizeof(double) * (r_shared ? mm : J * mm), hipMemcpyHostToDevice, d->stream));
    if (nu) HIPC(hipMemcpyAsync(sm + kScNu, nu, sizeof(double) * J * m, hipMemcpyHostToDevice, d->stream));
    double* ws = sp.spart_doubles > (size_t)ld * ld ? d->sc_ws : d->T;
    int* flags = reinterpret_cast<int*>(sm + kScFlag);
    HIPC(hipEventRecord(d->e0, d->stream));
    flush_pending(d);
    ekf::launch_dense64_score(sp, d->S, d->sc_H, ws, sm + kScR, r_shared ? 1 : 0, nu ? sm + kScNu : nullptr, J, m,
                              nis_out ? sm + kScNis : nullptr, sm + kScS, flags, d->stream);
    return finish_timed(d, elapsed_ms, {{nis_out, sm + kScNis, sizeof(double) * J},
                                        {S_out, sm + kScS, sizeof(double) * J * mm},
                                        {flag_out, flags, sizeof(int) * J}});
}

// The block-structured prediction: Fr, Qr and dx go up, one launch, timed by the handle's events.  The stored F and Q of
// the handle are not involved.
ekf_status dense64_propagate_block(ekf_dense64_s* d, int first, int r, const double* Fr, const double* Qr,
                                   const double* dx, double* elapsed_ms) {
    if (!d || !Fr || r < 1 || r > kMaxR || first < 0 || r > d->live || first > d->live - r)
        return fail(EKF_ERR_INVALID, "ekf_dense64_propagate_block: bad argument (the block must lie inside the live dimension)");
    HIPC(hipSetDevice(d->device));
    const size_t rr = sizeof(double) * r * r;
    HIPC(hipMemcpyAsync(d->blk_in, Fr, rr, hipMemcpyHostToDevice, d->stream));
    if (Qr) HIPC(hipMemcpyAsync(d->blk_in + kBlkQ, Qr, rr, hipMemcpyHostToDevice, d->stream));
    if (dx) HIPC(hipMemcpyAsync(d->blk_in + kBlkDx, dx, sizeof(double) * r, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    carry_or_flush(d, d->blk_in, nullptr, first, r, r);
    ekf::launch_dense64_block(d->S, d->x, d->blk_in, Qr ? d->blk_in + kBlkQ : nullptr, dx ? d->blk_in + kBlkDx : nullptr,
                              d->live, d->ld, first, r, d->stream);
    return finish_timed(d, elapsed_ms);
}

// ---- a Jacobian given by its s non-zero columns ---------------------------------------------------------------------------
constexpr int kMaxS = ekf::kDense64MaxS;
constexpr int kSparseRows = ekf::kDense64ScoreSparseMaxRows;

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

// One sparse correction: cols, Hc, R, nu go up into the (otherwise unused) operand buffer of the dense correction -- Hc and
// the list where its H would sit, R and nu in their usual places -- the verdict and nis come back in one copy.  Eager: the
// pending rows are applied first, four launches.  Deferred: three launches (no pass over Sigma) unless the m new rows do not
// fit; K and T stay in the pending panels, which the first call allocates (into a local: the member changes only when
// everything succeeded).
// The public entry point is checks | pend_reserve | uploads | e0 | correct_sparse_launch | correct_sparse_finish; a caller
// whose operands are already in the operand buffer (the landmark front end) runs the last two alone.
constexpr size_t kCsCols = (size_t)kMaxM * ekf::kDense64MaxS;   // the list behind Hc (64 ld >= 8192)
inline size_t cs_R(int ld) { return (size_t)2 * kMaxM * ld; }
inline size_t cs_nu(int ld) { return cs_R(ld) + kMaxM * kMaxM; }

ekf_status pend_reserve(ekf_dense64_s* d, const std::string& fn) {
    if (d->pend) return EKF_OK;
    const size_t bytes = sizeof(double) * (pend_zero(d->ld) + 2);
    double* fresh = nullptr;
    hipError_t e = hipMalloc((void**)&fresh, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(fresh, 0, bytes, d->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(d->stream);
        if (fresh) (void)hipFree(fresh);
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? EKF_ERR_NOMEM : EKF_ERR_HIP,
                    fn + ": " + hipGetErrorString(e) + " while reserving the pending panels");
    }
    d->pend = fresh;
    return EKF_OK;
}

// the launches of one correction on operands that sit in the operand buffer; behind e0
void correct_sparse_launch(ekf_dense64_s* d, bool deferred, int m, int s, bool have_nu) {
    const int ld = d->ld;
    const ekf::Dense64CorrectPlan& pl = d->pl_live;
    double* ws = d->ws_own ? d->ws_own : d->T;   // (the product buffer is dead between propagations)
    const int* dcols = reinterpret_cast<const int*>(d->corr_in + kCsCols);
    const double *dR = d->corr_in + cs_R(ld), *dnu = have_nu ? d->corr_in + cs_nu(ld) : nullptr;
    int* dverdict = reinterpret_cast<int*>(d->corr_out + 1);
    if (!deferred || d->pend_rows + m > kMaxP) flush_pending(d);   // deferred: only when there is no room for m more rows
    if (deferred)
        ekf::launch_dense64_correct_deferred(pl, d->S, d->x, ws, d->pend, d->pend + pend_T(ld), d->pend_rows, dcols,
                                             d->corr_in, dR, dnu, m, s, d->corr_out, dverdict, d->stream);
    else
        ekf::launch_dense64_correct_sparse(pl, d->S, d->x, ws, dcols, d->corr_in, dR, dnu, m, s, d->corr_out, dverdict,
                                           d->stream);
}

// the one synchronisation of a correction, its verdict, the count of the pending rows
ekf_status correct_sparse_finish(ekf_dense64_s* d, const std::string& fn, bool deferred, int m, double* nis_out,
                                 double* elapsed_ms) {
    double nis = 0.0;
    int verdict = 0;
    EKFC(finish_correction(d, elapsed_ms, &nis, &verdict));
    if (verdict != 0)
        return fail(EKF_ERR_STATE, fn + ": H Sigma H^T + R is singular or not finite (zero or non-finite pivot); " +
                                       (deferred ? "state, Sigma and the pending rows are unchanged"
                                                 : "state and Sigma are unchanged"));
    if (deferred) d->pend_rows += m;
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
    const int ld = d->ld;
    if (deferred) EKFC(pend_reserve(d, fn));
    HIPC(hipMemcpyAsync(d->corr_in, Hc, sizeof(double) * m * s, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(d->corr_in + kCsCols, cols, sizeof(int) * s, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(d->corr_in + cs_R(ld), R, sizeof(double) * m * m, hipMemcpyHostToDevice, d->stream));
    if (nu) HIPC(hipMemcpyAsync(d->corr_in + cs_nu(ld), nu, sizeof(double) * m, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    correct_sparse_launch(d, deferred, m, s, nu != nullptr);
    return correct_sparse_finish(d, fn, deferred, m, nis_out, elapsed_ms);
}

ekf_status dense64_flush(ekf_dense64_s* d, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_flush: null handle");
    if (elapsed_ms) *elapsed_ms = 0.0;
    if (d->pend_rows == 0) return EKF_OK;
    HIPC(hipSetDevice(d->device));
    HIPC(hipEventRecord(d->e0, d->stream));
    flush_pending(d);
    return finish_timed(d, elapsed_ms);
}

// Sparse scoring of J candidates: the operands go up into one buffer (allocated into a local, the members change only when
// that succeeded), one launch, the outputs come straight back into the caller's arrays.
// The public entry point is checks | sps_layout | sps_reserve | uploads | e0 | score_sparse_launch | copies back; a caller
// that builds the operands on the device (the landmark front end) writes them at the same offsets and launches the same.
struct SpsLayout {
    size_t oR, oNu, oNis, oS, oCols, oFlag, need;   // bytes from the buffer's start; Hc at 0
};
SpsLayout sps_layout(int J, int m, int s, bool r_shared, bool want_S) {
    const size_t mm = (size_t)m * m, al = 16;
    auto up = [&](size_t b) { return (b + al - 1) / al * al; };
    const size_t bHc = sizeof(double) * J * m * s, bR = sizeof(double) * (r_shared ? mm : J * mm);
    SpsLayout l;
    l.oR = up(bHc);
    l.oNu = l.oR + up(bR);
    l.oNis = l.oNu + up(sizeof(double) * J * m);
    l.oS = l.oNis + up(sizeof(double) * J);
    l.oCols = l.oS + (want_S ? up(sizeof(double) * J * mm) : 0);
    l.oFlag = l.oCols + up(sizeof(int) * J * s);
    l.need = l.oFlag + up(sizeof(int) * J);
    return l;
}
struct SpsView {
    double *Hc, *R, *nu, *nis, *S;
    int *cols, *flag;
};
SpsView sps_view(ekf_dense64_s* d, const SpsLayout& l, bool want_S) {
    char* b = d->sps;
    return {reinterpret_cast<double*>(b), reinterpret_cast<double*>(b + l.oR), reinterpret_cast<double*>(b + l.oNu),
            reinterpret_cast<double*>(b + l.oNis), want_S ? reinterpret_cast<double*>(b + l.oS) : nullptr,
            reinterpret_cast<int*>(b + l.oCols), reinterpret_cast<int*>(b + l.oFlag)};
}
ekf_status sps_reserve(ekf_dense64_s* d, size_t need, const char* fn) {
    if (need <= d->sps_bytes) return EKF_OK;
    char* fresh = nullptr;
    const hipError_t e = hipMalloc((void**)&fresh, need);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(e == hipErrorOutOfMemory ? EKF_ERR_NOMEM : EKF_ERR_HIP,
                    std::string(fn) + ": " + hipGetErrorString(e) + " while reserving the candidates' buffer");
    }
    if (d->sps) (void)hipFree(d->sps);   // (synchronises; no scoring call is in flight)
    d->sps = fresh;
    d->sps_bytes = need;
    return EKF_OK;
}
// the one launch on operands that sit in the buffer: eager, or read-through as rows are pending
void score_sparse_launch(ekf_dense64_s* d, const SpsView& v, int J, int m, int s, bool r_shared, bool have_nu,
                         bool want_nis) {
    const double* Tq = d->pend_rows ? d->pend + pend_T(d->ld) : nullptr;   // (no panels before the first deferred call)
    ekf::launch_dense64_score_sparse(d->S, d->pend, Tq, d->pend_rows, v.cols, v.Hc, v.R, r_shared ? 1 : 0,
                                     have_nu ? v.nu : nullptr, J, m, s, d->ld, want_nis ? v.nis : nullptr, v.S, v.flag,
                                     nullptr, d->stream);
}

ekf_status dense64_score_sparse(ekf_dense64_s* d, int J, int m, int s, const int* cols, const double* Hc, const double* R,
                                int r_shared, const double* nu, double* nis_out, double* S_out, int* flag_out,
                                double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_score_sparse: null handle");
    if (!cols || !Hc || !R || J < 1 || m < 1 || m > kMaxM || m > d->live || s < 1 || s > kMaxS || s > d->live ||
        (long long)J * m > kSparseRows || (nis_out && !nu) || (!nis_out && !S_out && !flag_out))
        return fail(EKF_ERR_INVALID, "ekf_dense64_score_sparse: bad argument");
    if (!index_lists_ok(d->host_stamp, d->live, J, s, cols))
        return fail(EKF_ERR_INVALID, "ekf_dense64_score_sparse: every row of cols must hold distinct indices in [0, N), "
                                     "below the live dimension");
    HIPC(hipSetDevice(d->device));
    const size_t mm = (size_t)m * m;
    const SpsLayout l = sps_layout(J, m, s, r_shared != 0, S_out != nullptr);
    EKFC(sps_reserve(d, l.need, "ekf_dense64_score_sparse"));
    const SpsView v = sps_view(d, l, S_out != nullptr);
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

// ---- (re)initialisation of a block of states, block readouts, state slices ----------------------------------------------
// G, W, xb and the list go up into the buffer allocated with the handle, one launch, timed by the handle's events.  The
// stored F and Q of the handle are not involved.
// the launches on operands that sit in the buffer (the public call after its uploads, the landmark front end after
// k_dlm_decide): the pending rows carried or applied, then the one launch; behind e0
void init_block_launch(ekf_dense64_s* d, int first, int r, int s, bool have_W, bool have_xb) {
    double* in = d->ini_in;
    int* dcols = reinterpret_cast<int*>(in + kIniCols);
    carry_or_flush(d, in, s > 0 ? dcols : nullptr, first, r, s);
    ekf::launch_dense64_init(d->S, d->x, dcols, in, have_W ? in + kIniW : nullptr, have_xb ? in + kIniXb : nullptr, d->live,
                             d->ld, first, r, s, d->stream);
}

ekf_status dense64_init_block(ekf_dense64_s* d, int first, int r, int s, const int* cols, const double* G, const double* W,
                              const double* xb, double* elapsed_ms) {
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
    double* in = d->ini_in;
    int* dcols = reinterpret_cast<int*>(in + kIniCols);
    if (s > 0) {
        HIPC(hipMemcpyAsync(in, G, sizeof(double) * r * s, hipMemcpyHostToDevice, d->stream));
        HIPC(hipMemcpyAsync(dcols, cols, sizeof(int) * s, hipMemcpyHostToDevice, d->stream));
    }
    if (W) HIPC(hipMemcpyAsync(in + kIniW, W, sizeof(double) * r * r, hipMemcpyHostToDevice, d->stream));
    if (xb) HIPC(hipMemcpyAsync(in + kIniXb, xb, sizeof(double) * r, hipMemcpyHostToDevice, d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    init_block_launch(d, first, r, s, W != nullptr, xb != nullptr);
    return finish_timed(d, elapsed_ms);
}

// The exchange of two blocks: nothing goes up.  The pending rows take the same permutation (a congruence with A = P, the
// algebra of carry_or_flush) when the handle carries them, and are applied first otherwise.
ekf_status dense64_swap_blocks(ekf_dense64_s* d, int first_a, int first_b, int r, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_swap_blocks: null handle");
    if (r < 1 || r > kMaxR || r > d->live || first_a < 0 || first_b < 0 || first_a > d->live - r || first_b > d->live - r)
        return fail(EKF_ERR_INVALID, "ekf_dense64_swap_blocks: bad argument (both blocks must lie inside the live dimension)");
    if (std::abs(first_a - first_b) < r)
        return fail(EKF_ERR_INVALID, "ekf_dense64_swap_blocks: the blocks must be disjoint, |first_a - first_b| >= r");
    HIPC(hipSetDevice(d->device));
    HIPC(hipEventRecord(d->e0, d->stream));
    if (d->carry && d->pend_rows > 0)
        ekf::launch_dense64_panel_swap(d->pend, d->pend + pend_T(d->ld), d->pend_rows, d->ld, first_a, first_b, r, d->stream);
    else
        flush_pending(d);
    ekf::launch_dense64_swap(d->S, d->x, d->live, d->ld, first_a, first_b, r, d->stream);
    return finish_timed(d, elapsed_ms);
}

// out[a][c] = Sigma[rows[a]][cols[c]]: the two lists go up, one gather launch into the handle's buffer, one copy back.
ekf_status dense64_get_sigma_block(ekf_dense64_s* d, int nr, const int* rows, int nc, const int* cols, double* out) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_get_sigma_block: null handle");
    if (!rows || !cols || !out || nr < 1 || nc < 1 || (long long)nr * nc > kReadMax)
        return fail(EKF_ERR_INVALID, "ekf_dense64_get_sigma_block: bad argument");
    for (int a = 0; a < nr; a++)
        if (rows[a] < 0 || rows[a] >= d->N)
            return fail(EKF_ERR_INVALID, "ekf_dense64_get_sigma_block: every index of rows must lie in [0, N)");
    for (int c = 0; c < nc; c++)
        if (cols[c] < 0 || cols[c] >= d->N)
            return fail(EKF_ERR_INVALID, "ekf_dense64_get_sigma_block: every index of cols must lie in [0, N)");
    HIPC(hipSetDevice(d->device));
    int *drows = reinterpret_cast<int*>(d->rd_buf + kRdRows), *dcols = reinterpret_cast<int*>(d->rd_buf + kRdCols);
    HIPC(hipMemcpyAsync(drows, rows, sizeof(int) * nr, hipMemcpyHostToDevice, d->stream));
    HIPC(hipMemcpyAsync(dcols, cols, sizeof(int) * nc, hipMemcpyHostToDevice, d->stream));
    if (d->carry && d->pend_rows > 0) {   // Sigma_cur through the pending rows; read-only
        ekf::launch_dense64_read_block_deferred(d->S, d->pend, d->pend + pend_T(d->ld), d->pend_rows, drows, dcols,
                                                d->rd_buf, nr, nc, d->ld, d->N, d->live, d->stream);
    } else {
        flush_pending(d);
        ekf::launch_dense64_read_block(d->S, drows, dcols, d->rd_buf, nr, nc, d->ld, d->stream);
    }
    HIPC(hipGetLastError());
    HIPC(hipMemcpyAsync(out, d->rd_buf, sizeof(double) * nr * nc, hipMemcpyDeviceToHost, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}

ekf_status dense64_state_block(const char* name, ekf_dense64_s* d, int first, int count, double* out, const double* x) {
    if (!d) return fail(EKF_ERR_INVALID, std::string(name) + ": null handle");
    if ((!out && !x) || count < 1 || first < 0 || count > d->N || first > d->N - count)
        return fail(EKF_ERR_INVALID, std::string(name) + ": bad argument");
    HIPC(hipSetDevice(d->device));
    if (out) HIPC(hipMemcpyAsync(out, d->x + first, sizeof(double) * count, hipMemcpyDeviceToHost, d->stream));
    else HIPC(hipMemcpyAsync(d->x + first, x, sizeof(double) * count, hipMemcpyHostToDevice, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}

// The live dimension.  Growing: a pending row is zero on [old, ld) whatever the panels hold there from wider calls, so those
// columns of the p waiting rows of both panels are set to zero -- up to the new width rounded up to 128, what the calls of
// that width keep zero -- and nothing is flushed.  Shrinking: the rows have support up to the old width, so they are applied
// first, at the old width.
ekf_status dense64_set_live(ekf_dense64_s* d, int Na) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_set_live: null handle");
    if (Na < 1 || Na > d->N) return fail(EKF_ERR_INVALID, "ekf_dense64_set_live: the live dimension must lie in [1, N]");
    if (Na == d->live) return EKF_OK;
    if (d->pend_rows > 0) {
        HIPC(hipSetDevice(d->device));
        if (Na < d->live) {
            flush_pending(d);
        } else {
            const int upto = std::min(d->ld, round_up(Na, ekf::kDenseTile));
            for (double* panel : {d->pend, d->pend + pend_T(d->ld)})
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

// One streaming launch over the two rectangles; the two result words sit where a correction's nis and verdict do.
ekf_status dense64_coupling(ekf_dense64_s* d, int Na, long long* nonzero, double* max_abs, double* elapsed_ms) {
    if (!d || !nonzero) return fail(EKF_ERR_INVALID, "ekf_dense64_coupling: null argument");
    if (Na < 1 || Na > d->N) return fail(EKF_ERR_INVALID, "ekf_dense64_coupling: Na must lie in [1, N]");
    HIPC(hipSetDevice(d->device));
    static_assert(sizeof(unsigned long long) == sizeof(double), "two words in corr_out");
    unsigned long long out[2] = {0, 0};
    HIPC(hipMemsetAsync(d->corr_out, 0, sizeof(out), d->stream));
    HIPC(hipEventRecord(d->e0, d->stream));
    flush_pending(d);
    ekf::launch_dense64_coupling(d->S, d->N, d->ld, Na, reinterpret_cast<unsigned long long*>(d->corr_out), d->stream);
    EKFC(finish_timed(d, elapsed_ms, {{out, d->corr_out, sizeof(out)}}));
    *nonzero = (long long)out[0];
    if (max_abs) std::memcpy(max_abs, &out[1], sizeof(double));
    return EKF_OK;
}

// ---- the landmark front end: the reference's model and decision rule on the handle's own state -------------------------
ekf::Params landmark_params(const ekf_params* params) {
    ekf_params p;
    ekf_default_params(&p);
    if (params) p = *params;
    return ekf::Params{p.sigma0_landmark, p.q_pose, p.r_meas, p.gate_new, p.gate_update, p.straight_eps};
}

// calculate_maha_dis (:217-276) of one reading: k_dlm_terms writes the operands where the uploads of score_sparse would
// put them, then that call's one launch; everything asked for comes back behind the one synchronisation.
ekf_status dense64_score_landmarks(ekf_dense64_s* d, const ekf_params* params, double sx, double sy, int first_lm, int count,
                                   double* nis_out, double* S_out, int* flag_out, int* cols_out, double* Hc_out,
                                   double* nu_out, double* elapsed_ms) {
    if (!d) return fail(EKF_ERR_INVALID, "ekf_dense64_score_landmarks: null handle");
    if (count < 1 || count > kSparseRows / 2 || first_lm < 0 || 3 + 2 * ((long long)first_lm + count) > d->live ||
        (!nis_out && !S_out && !flag_out))
        return fail(EKF_ERR_INVALID, "ekf_dense64_score_landmarks: bad argument (the landmarks must lie inside the live "
                                     "dimension)");
    const ekf::Params p = landmark_params(params);
    HIPC(hipSetDevice(d->device));
    const SpsLayout l = sps_layout(count, 2, 5, true, S_out != nullptr);
    EKFC(sps_reserve(d, l.need, "ekf_dense64_score_landmarks"));
    const SpsView v = sps_view(d, l, S_out != nullptr);
    HIPC(hipEventRecord(d->e0, d->stream));
    ekf::launch_dense64_lm_terms(d->x, sx, sy, first_lm, count, 0, p.r_meas, v.cols, v.Hc, v.R, v.nu, d->stream);
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
ekf_status dense64_associate_landmarks(ekf_dense64_s* d, const ekf_params* params, int J, const double* meas_xy, int n_max,
                                       int* known, unsigned flags, int* assoc_out, double* best_out, double* elapsed_ms) {
    const std::string fn = "ekf_dense64_associate_landmarks";
    if (!d) return fail(EKF_ERR_INVALID, fn + ": null handle");
    if (!known || !meas_xy) return fail(EKF_ERR_INVALID, fn + ": null argument");
    if (J < 1) return fail(EKF_ERR_INVALID, fn + ": J must be at least 1");
    if (n_max < 0 || 3 + 2 * (long long)n_max > d->N)
        return fail(EKF_ERR_INVALID, fn + ": n_max must lie in [0, (N - 3) / 2]");
    if (*known < 0 || *known > n_max) return fail(EKF_ERR_INVALID, fn + ": *known must lie in [0, n_max]");
    if (3 + 2 * *known > d->live)
        return fail(EKF_ERR_INVALID, fn + ": the known landmarks must lie inside the live dimension");
    if (flags & ~(EKF_DENSE64_LM_DEFERRED | EKF_DENSE64_LM_GROW_LIVE))
        return fail(EKF_ERR_INVALID, fn + ": unknown flag bits");
    const bool deferred = (flags & EKF_DENSE64_LM_DEFERRED) != 0;
    const ekf::Params p = landmark_params(params);
    if (elapsed_ms) *elapsed_ms = 0.0;
    for (int j = 0; j < J; j++) {
        if (assoc_out) assoc_out[j] = -2;
        if (best_out) best_out[j] = p.gate_new;
    }
    HIPC(hipSetDevice(d->device));
    if (!d->lm_rec) {
        ekf::Dense64LmRecord* fresh = nullptr;
        const hipError_t e = hipMalloc((void**)&fresh, sizeof(*fresh));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? EKF_ERR_NOMEM : EKF_ERR_HIP,
                        fn + ": " + hipGetErrorString(e) + " while reserving the decision record");
        }
        d->lm_rec = fresh;
    }
    if (deferred) EKFC(pend_reserve(d, fn));
    // the scoring buffer once, for the full map: a map that is being discovered must not pay a hipMalloc and a hipFree
    // (a device synchronisation) per new landmark
    if (n_max > 0) EKFC(sps_reserve(d, sps_layout(n_max, 2, 5, true, false).need, fn.c_str()));
    double total = 0.0, ms = 0.0;
    double* pms = elapsed_ms ? &ms : nullptr;
    for (int j = 0; j < J; j++) {
        const double sx = meas_xy[2 * j], sy = meas_xy[2 * j + 1];
        const int k = *known;
        SpsView v{};
        if (k > 0) v = sps_view(d, sps_layout(k, 2, 5, true, false), false);   // (k <= n_max: inside the buffer)
        HIPC(hipEventRecord(d->e0, d->stream));
        if (k > 0) {
            ekf::launch_dense64_lm_terms(d->x, sx, sy, 0, k, 0, p.r_meas, v.cols, v.Hc, v.R, v.nu, d->stream);
            score_sparse_launch(d, v, k, 2, 5, true, true, true);
        }
        ekf::launch_dense64_lm_decide(v.nis, k, k, n_max, p.gate_new, p.gate_update, p.sigma0_landmark, d->x, sx, sy,
                                      d->lm_rec, d->ini_in + kIniW, d->ini_in + kIniXb, d->stream);
        ekf::Dense64LmRecord rec{};
        EKFC(finish_timed(d, pms, {{&rec, d->lm_rec, sizeof(rec)}}));
        total += ms;
        if (elapsed_ms) *elapsed_ms = total;
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
            EKFC(dense64_set_live(d, 3 + 2 * (k + 1)));
        }
        HIPC(hipEventRecord(d->e0, d->stream));
        if (fresh_lm) init_block_launch(d, 3 + 2 * k, 2, 0, true, true);   // s = 0, W = sigma0 I, xb
        if (!corrects) {   // (a gate_update <= 0: the landmark is initialised and not corrected)
            EKFC(finish_timed(d, pms));
            total += ms;
            if (elapsed_ms) *elapsed_ms = total;
            *known = k + 1;
            if (assoc_out) assoc_out[j] = -1;
            continue;
        }
        // the winner's operands from the current state, that is after an initialisation; the innovation wrapped (:183)
        ekf::launch_dense64_lm_terms(d->x, sx, sy, rec.win, 1, 1, p.r_meas, reinterpret_cast<int*>(d->corr_in + kCsCols),
                                     d->corr_in, d->corr_in + cs_R(d->ld), d->corr_in + cs_nu(d->ld), d->stream);
        correct_sparse_launch(d, deferred, 2, 5, true);
        ekf::launch_dense64_lm_wrap(d->x, reinterpret_cast<const int*>(d->corr_out + 1), d->stream);   // :187 / :385
        if (assoc_out) assoc_out[j] = -1;
        ms = 0.0;
        const ekf_status st = correct_sparse_finish(d, fn, deferred, 2, nullptr, pms);
        if (fresh_lm && (st == EKF_OK || st == EKF_ERR_STATE)) *known = k + 1;   // the initialisation stands
        total += ms;   // (a refused correction's launches ran and were timed)
        if (elapsed_ms) *elapsed_ms = total;
        if (st != EKF_OK) return st;
        if (assoc_out) assoc_out[j] = rec.win;
    }
    return EKF_OK;
}

}  // namespace

extern "C" {

ekf_status ekf_dense_create(int N, int device, ekf_dense_handle* out) {
    return dense_create<ekf_dense_s, DenseOps32>("ekf_dense_create", N, device, out);
}
ekf_status ekf_dense_destroy(ekf_dense_handle d) { return dense_destroy(d); }
ekf_status ekf_dense_set(ekf_dense_handle d, const float* F, const float* Sigma, const float* Q) {
    return dense_set(d, F, Sigma, Q);
}
ekf_status ekf_dense_propagate(ekf_dense_handle d, int iterations, double* elapsed_ms) {
    return dense_propagate<DenseOps32>("ekf_dense_propagate", d, iterations, elapsed_ms);
}
ekf_status ekf_dense_launch_info(ekf_dense_handle d, int* ld, int* tiles, int* n_big, int* n_tail) {
    return dense_launch_info<DenseOps32>(d, ld, tiles, n_big, n_tail);
}
ekf_status ekf_dense_tile_map(ekf_dense_handle d, unsigned char* map) { return dense_tile_map<DenseOps32>(d, map); }
ekf_status ekf_dense_get_sigma(ekf_dense_handle d, float* out) { return dense_get_sigma(d, out); }

ekf_status ekf_dense64_create(int N, int device, ekf_dense64_handle* out) {
    return dense_create<ekf_dense64_s, DenseOps64>("ekf_dense64_create", N, device, out);
}
ekf_status ekf_dense64_destroy(ekf_dense64_handle d) { return dense_destroy(d); }
ekf_status ekf_dense64_set(ekf_dense64_handle d, const double* F, const double* Sigma, const double* Q) {
    return dense_set(d, F, Sigma, Q);
}
ekf_status ekf_dense64_propagate(ekf_dense64_handle d, int iterations, double* elapsed_ms) {
    return dense_propagate<DenseOps64>("ekf_dense64_propagate", d, iterations, elapsed_ms);
}
ekf_status ekf_dense64_launch_info(ekf_dense64_handle d, int* ld, int* tiles, int* n_big, int* n_tail) {
    return dense_launch_info<DenseOps64>(d, ld, tiles, n_big, n_tail);
}
ekf_status ekf_dense64_tile_map(ekf_dense64_handle d, unsigned char* map) { return dense_tile_map<DenseOps64>(d, map); }
ekf_status ekf_dense64_get_sigma(ekf_dense64_handle d, double* out) { return dense_get_sigma(d, out); }
ekf_status ekf_dense64_set_state(ekf_dense64_handle d, const double* x) {
    if (!d || !x) return fail(EKF_ERR_INVALID, "ekf_dense64_set_state: null argument");
    HIPC(hipSetDevice(d->device));
    HIPC(hipMemcpyAsync(d->x, x, sizeof(double) * d->N, hipMemcpyHostToDevice, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}
ekf_status ekf_dense64_get_state(ekf_dense64_handle d, double* out) {
    if (!d || !out) return fail(EKF_ERR_INVALID, "ekf_dense64_get_state: null argument");
    HIPC(hipSetDevice(d->device));
    HIPC(hipMemcpyAsync(out, d->x, sizeof(double) * d->N, hipMemcpyDeviceToHost, d->stream));
    HIPC(hipStreamSynchronize(d->stream));
    return EKF_OK;
}
ekf_status ekf_dense64_correct(ekf_dense64_handle d, int m, const double* H, const double* R, const double* nu,
                               double* nis_out, double* elapsed_ms) {
    return dense64_correct(d, m, H, R, nu, nis_out, elapsed_ms);
}
ekf_status ekf_dense64_score(ekf_dense64_handle d, int J, int m, const double* H, const double* R, int r_shared,
                             const double* nu, double* nis_out, double* S_out, int* flag_out, double* elapsed_ms) {
    return dense64_score(d, J, m, H, R, r_shared, nu, nis_out, S_out, flag_out, elapsed_ms);
}
ekf_status ekf_dense64_propagate_block(ekf_dense64_handle d, int first, int r, const double* Fr, const double* Qr,
                                       const double* dx, double* elapsed_ms) {
    return dense64_propagate_block(d, first, r, Fr, Qr, dx, elapsed_ms);
}
ekf_status ekf_dense64_correct_sparse(ekf_dense64_handle d, int m, int s, const int* cols, const double* Hc,
                                      const double* R, const double* nu, double* nis_out, double* elapsed_ms) {
    return dense64_correct_sparse(d, false, m, s, cols, Hc, R, nu, nis_out, elapsed_ms);
}
ekf_status ekf_dense64_correct_sparse_deferred(ekf_dense64_handle d, int m, int s, const int* cols, const double* Hc,
                                               const double* R, const double* nu, double* nis_out, double* elapsed_ms) {
    return dense64_correct_sparse(d, true, m, s, cols, Hc, R, nu, nis_out, elapsed_ms);
}
ekf_status ekf_dense64_flush(ekf_dense64_handle d, double* elapsed_ms) { return dense64_flush(d, elapsed_ms); }
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
ekf_status ekf_dense64_set_live(ekf_dense64_handle d, int Na) { return dense64_set_live(d, Na); }
ekf_status ekf_dense64_get_live(ekf_dense64_handle d, int* Na) {
    if (!d || !Na) return fail(EKF_ERR_INVALID, "ekf_dense64_get_live: null argument");
    *Na = d->live;
    return EKF_OK;
}
ekf_status ekf_dense64_coupling(ekf_dense64_handle d, int Na, long long* nonzero, double* max_abs, double* elapsed_ms) {
    return dense64_coupling(d, Na, nonzero, max_abs, elapsed_ms);
}
ekf_status ekf_dense64_score_sparse(ekf_dense64_handle d, int J, int m, int s, const int* cols, const double* Hc,
                                    const double* R, int r_shared, const double* nu, double* nis_out, double* S_out,
                                    int* flag_out, double* elapsed_ms) {
    return dense64_score_sparse(d, J, m, s, cols, Hc, R, r_shared, nu, nis_out, S_out, flag_out, elapsed_ms);
}
ekf_status ekf_dense64_score_landmarks(ekf_dense64_handle d, const ekf_params* params, double sx, double sy, int first_lm,
                                       int count, double* nis_out, double* S_out, int* flag_out, int* cols_out,
                                       double* Hc_out, double* nu_out, double* elapsed_ms) {
    return dense64_score_landmarks(d, params, sx, sy, first_lm, count, nis_out, S_out, flag_out, cols_out, Hc_out, nu_out,
                                   elapsed_ms);
}
ekf_status ekf_dense64_associate_landmarks(ekf_dense64_handle d, const ekf_params* params, int J, const double* meas_xy,
                                           int n_max, int* known, unsigned flags, int* assoc_out, double* best_out,
                                           double* elapsed_ms) {
    return dense64_associate_landmarks(d, params, J, meas_xy, n_max, known, flags, assoc_out, best_out, elapsed_ms);
}
ekf_status ekf_dense64_init_block(ekf_dense64_handle d, int first, int r, int s, const int* cols, const double* G,
                                  const double* W, const double* xb, double* elapsed_ms) {
    return dense64_init_block(d, first, r, s, cols, G, W, xb, elapsed_ms);
}
ekf_status ekf_dense64_swap_blocks(ekf_dense64_handle d, int first_a, int first_b, int r, double* elapsed_ms) {
    return dense64_swap_blocks(d, first_a, first_b, r, elapsed_ms);
}
ekf_status ekf_dense64_get_sigma_block(ekf_dense64_handle d, int nr, const int* rows, int nc, const int* cols,
                                       double* out) {
    return dense64_get_sigma_block(d, nr, rows, nc, cols, out);
}
ekf_status ekf_dense64_get_state_block(ekf_dense64_handle d, int first, int count, double* out) {
    return dense64_state_block("ekf_dense64_get_state_block", d, first, count, out, nullptr);
}
ekf_status ekf_dense64_set_state_block(ekf_dense64_handle d, int first, int count, const double* x) {
    return dense64_state_block("ekf_dense64_set_state_block", d, first, count, nullptr, x);
}

}  // extern "C"
