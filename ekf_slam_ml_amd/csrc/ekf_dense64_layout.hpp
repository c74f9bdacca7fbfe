// ekf_dense64_layout.hpp -- where every operand of the fp64 dense handle (ekf_dense64_s, ekf_dense_handle.hpp) sits inside
// its device buffer: per buffer one function of what the layout depends on, returning byte offsets from the buffer's start
// and the total size.  Pure arithmetic, nothing from HIP: tests/cpp/dense64_layout_dump.cpp prints every layout on a CPU
// and tests/test_dense64_layout_host.py checks offsets, overlap and alignment.  The kernels rely on these offsets (16-byte
// boundaries of Hc and nu, f64x4 reads); the typed pointers made from them are the views of ekf_dense_handle.hpp.
#pragma once
#include <stddef.h>

namespace ekf {
// the limits of the handle's calls (include/ekfslam.h: EKF_DENSE64_*)
constexpr int kDense64MaxM = 64;                     // rows of one correction's Jacobian
constexpr int kDense64ScoreMaxRows = 2048;           // J * m of one dense scoring call
constexpr int kDense64MaxR = 64;                     // states of one block
constexpr int kDense64MaxS = 64;                     // listed columns of a sparse Jacobian
constexpr int kDense64ScoreSparseMaxRows = 65536;    // J * m of one sparse scoring call
constexpr int kDense64PendingMaxRows = 64;           // rows of K and T that wait for the flush
constexpr int kDense64ReadMax = 65536;               // entries of one block readout
constexpr int kDense64ScanMaxBeams = 1024;           // beams of one laser scan
constexpr int kDense64ScanMaxClusters = 128;         // clusters of one scan, and the most circles a call returns
constexpr int kDense64JointMaxReadings = 128;        // readings of one joint association (= kDense64ScanMaxClusters)
constexpr int kDense64JointMaxPairs = 30;            // pairs of one stacked correction: m = 2 V <= 64 and s = 3 + 2 V <= 64
constexpr int kDense64JointInitGroup = 32;           // new landmarks of one initialisation: r = 2 n <= 64
constexpr int kDense64JcbbMaxReadings = 32;          // readings of one joint compatibility association
constexpr int kDense64JcbbMaxCand = 4;               // candidates of a reading: P <= 128, W <= 256 x 256
constexpr int kDense64JcbbTile = 16;                 // k_jc_cross: a workgroup computes 16 x 16 blocks W[p][q]

namespace d64 {
constexpr size_t kF = sizeof(double), kI = sizeof(int), kM = kDense64MaxM, kR = kDense64MaxR, kS = kDense64MaxS;

// corr_in as the dense correction sees it: H [64][ld] | H^T [ld][m rounded up to 16] (room for 64) | R [64 * 64] | nu [64]
struct CorrInLayout { size_t H, Ht, R, nu, bytes; };
inline CorrInLayout corr_in_layout(int ld) { const size_t Ht = kF * kM * ld, R = 2 * Ht, nu = R + kF * kM * kM; return {0, Ht, R, nu, nu + kF * kM}; }
// ... and as the sparse correction sees it: Hc [64][64] and the list [64] behind it where H would sit (64 ld >= 8192), R and
// nu in their usual places
struct CorrSparseLayout { size_t Hc, cols, R, nu, bytes; };
inline CorrSparseLayout corr_sparse_layout(int ld) { const CorrInLayout d = corr_in_layout(ld); return {0, kF * kM * kS, d.R, d.nu, d.bytes}; }
// corr_out: nis | verdict (an int in the second double); the two 64-bit words of the coupling count sit on the same two
struct CorrOutLayout { size_t nis, verdict, bytes; };
inline CorrOutLayout corr_out_layout() { return {0, kF, 2 * kF}; }
// sc_small: R [2048 * 64] | nu [2048] | nis [2048] | S [2048 * 64] | flags (ints) [2048]
struct ScSmallLayout { size_t R, nu, nis, S, flag, bytes; };
inline ScSmallLayout sc_small_layout() {
    const size_t rows = kDense64ScoreMaxRows, nu = kF * rows * kM, nis = nu + kF * rows, S = nis + kF * rows,
                 flag = S + kF * rows * kM;
    return {0, nu, nis, S, flag, flag + kF * (rows / 2)};
}
// blk_in: Fr [64 * 64] | Qr [64 * 64] | dx [64]
struct BlkInLayout { size_t Fr, Qr, dx, bytes; };
inline BlkInLayout blk_in_layout() { return {0, kF * kR * kR, 2 * kF * kR * kR, 2 * kF * kR * kR + kF * kR}; }
// ini_in: G [64 * 64] | W [64 * 64] | xb [64] | cols (ints) [64]
struct IniInLayout { size_t G, W, xb, cols, bytes; };
inline IniInLayout ini_in_layout() { const size_t W = kF * kR * kS, xb = W + kF * kR * kR, cols = xb + kF * kR; return {0, W, xb, cols, cols + kF * (kS / 2)}; }
// rd_buf: out [65536] | rows (ints) [65536] | cols (ints) [65536]
struct RdBufLayout { size_t out, rows, cols, bytes; };
inline RdBufLayout rd_buf_layout() { const size_t n = kDense64ReadMax, rows = kF * n, cols = rows + kF * (n / 2); return {0, rows, cols, cols + kF * (n / 2)}; }
// the pending panels: K^T [64][ld] | T [64][ld] | a word kept at zero (the flush's verdict argument)
struct PendLayout { size_t K, T, zero, bytes; };
inline PendLayout pend_layout(int ld) { const size_t T = kF * kDense64PendingMaxRows * ld; return {0, T, 2 * T, 2 * T + 2 * kF}; }
// the one buffer of a sparse scoring call, cut per call: Hc | R | nu | nis | S | cols (ints) | flags (ints), every region
// on a 16-byte boundary, S only when it is asked for
struct SpsLayout { size_t Hc, R, nu, nis, S, cols, flag, bytes; };
inline SpsLayout sps_layout(int J, int m, int s, bool r_shared, bool want_S) {
    const size_t mm = (size_t)m * m, al = 16;
    auto up = [&](size_t b) { return (b + al - 1) / al * al; };
    const size_t R = up(kF * J * m * s), nu = R + up(kF * (r_shared ? mm : J * mm)), nis = nu + up(kF * J * m),
                 S = nis + up(kF * J), cols = S + (want_S ? up(kF * J * mm) : 0), flag = cols + up(kI * J * s);
    return {0, R, nu, nis, S, cols, flag, flag + up(kI * J)};
}
// ekf_dense64_measure_landmarks' view of that same buffer (it scores nothing): the pose captured at the top of the call
// (3 doubles in a 32-byte slot) | the call's readings [n_lm][2], on a 16-byte boundary, when the first call initialises
struct LmMeasureLayout { size_t pose, xy, bytes; };
inline LmMeasureLayout lm_measure_layout(int n_lm) { return {0, 4 * kF, 4 * kF + 2 * kF * (size_t)n_lm}; }
// scan: ranges [1024] | the record that comes down in one copy: head (ints: circles kept, clusters) | centres [128][2] |
// radii [128] | every cluster's x, y, r, is_circle [128][4], which comes down only when it is asked for
struct ScanLayout { size_t ranges, head, centres, radii, all, bytes, record_bytes; };
inline ScanLayout scan_layout() {
    const size_t nb = kDense64ScanMaxBeams, nc = kDense64ScanMaxClusters, head = kF * nb, centres = head + 2 * kI,
                 radii = centres + kF * 2 * nc, all = radii + kF * nc;
    return {0, head, centres, radii, all, all + kF * 4 * nc, all - head};
}
// the joint association: the readings [128][2] as they went up | the per-reading records of k_djt_argmin [128] (32 bytes each)
// | what comes down in one copy: head (ints: n_match, n_new, n_pairs, 0) | the final records [128] | the stacked xb [128][2] |
// and what stays on the device: the pairs' landmarks and readings (ints) [128] each | W = sigma0 I at r = 64 | W at the
// r < 64 of the last initialisation group.  Every region on a 16-byte boundary.
struct JointLayout { size_t xy, pre, head, rec, xb, pair_lm, pair_j, W_full, W_last, bytes, record_bytes; };
inline JointLayout joint_layout() {
    const size_t nj = kDense64JointMaxReadings, rb = 32, pre = 2 * kF * nj, head = pre + rb * nj, rec = head + 4 * kI,
                 xb = rec + rb * nj, pair_lm = xb + 2 * kF * nj, pair_j = pair_lm + kI * nj, W_full = pair_j + kI * nj,
                 W_last = W_full + kF * kR * kR;
    return {0, pre, head, rec, xb, pair_lm, pair_j, W_full, W_last, W_last + kF * kR * kR, pair_lm - head};
}
// the joint compatibility association (ekf_dense64_jcbb.hip), cut for its maxima (32 readings, 4 candidates each, P <= 128):
// what comes down in one copy: head (ints: P, 0, 0, 0) | cand_count [32] | offset [32] | is_new [32] | cand_lm [32][4] |
// reading_of [128] | lm_of [128] (ints) | best [32] | cand_nis [32][4] | nu [128][2]; then what stays on the device: cols
// [128][5] (ints) | Hc [128][2][5]; then W [P][P][2][2] at the call's own P (512 KB at P = 128), on a 32-byte boundary
struct JcbbLayout { size_t head, cand_count, offset, is_new, cand_lm, reading_of, lm_of, best, cand_nis, nu, cols, Hc, W, bytes, record_bytes; };
inline JcbbLayout jcbb_layout() {
    const size_t nj = 32, nc = 4, np = nj * nc, cand_count = 4 * kI, offset = cand_count + kI * nj, is_new = offset + kI * nj,
                 cand_lm = is_new + kI * nj, reading_of = cand_lm + kI * np, lm_of = reading_of + kI * np,
                 best = lm_of + kI * np, cand_nis = best + kF * nj, nu = cand_nis + kF * np, cols = nu + 2 * kF * np,
                 Hc = cols + kI * 5 * np, W = (Hc + 10 * kF * np + 31) / 32 * 32;
    return {0, cand_count, offset, is_new, cand_lm, reading_of, lm_of, best, cand_nis, nu, cols, Hc, W, W + 4 * kF * np * np, cols};
}
}  // namespace d64

// ---- map joining (ekf_dense64_join.hip; the definition is include/ekfslam.h's, ekf_dense64_join_congruence): launch geometry
// and the workspace, which comes from the DESTINATION's ledger.  Offsets in doubles: the old pose rows P [3][ld] (their first
// three columns are Sigma_pp) | the old pose columns Pc, transposed [3][ld] | terms = G [4] | E [Nb][3] | W = E Sigma_pp
// [Nb][3] | the new pose [3] (then one double of padding).  Na, Nb odd and >= 3, Na + Nb - 3 <= the destination's N.
constexpr int kDense64JoinTileRows = 64;    // the hot pass: tiles of the SOURCE's Sigma[3:Nb, 3:Nb], origins on odd indices
constexpr int kDense64JoinTileCols = 128;
constexpr int kDense64JoinThreads = 256;
constexpr int kDense64JoinCrossRows = 8;    // the two rectangles: a workgroup writes 8 rows of 512 columns
constexpr int kDense64JoinCrossCols = 2 * kDense64JoinThreads;
struct Dense64JoinPlan {
    int Na, Nb, Nj, ld_dst, ld_src;      // Nj = Na + Nb - 3, the joined live dimension
    int pairs_dst, pairs_src, pairs_j;   // index 0 and the pairs (1, 2), (3, 4), ... below Na, Nb, Nj
    int corner_gx, corner_gy;            // k_jn_corner's grid (0 x 0 at Nb = 3: not launched)
    int rows_gx, rows_gy;                // k_jn_cross, X_rows[3:, 3:Na]: (Nb - 3) rows of (Na - 3) columns
    int cols_gx, cols_gy;                // k_jn_cross, X_cols[3:Na, 3:]: (Na - 3) rows of (Nb - 3) columns
    size_t off_rows, off_cols, off_terms, off_W, off_pose, doubles;
};
inline Dense64JoinPlan dense64_join_plan(int Na, int ld_dst, int Nb, int ld_src) {
    Dense64JoinPlan p{};
    p.Na = Na, p.Nb = Nb, p.Nj = Na + Nb - 3, p.ld_dst = ld_dst, p.ld_src = ld_src;
    p.pairs_dst = (Na + 1) / 2, p.pairs_src = (Nb + 1) / 2, p.pairs_j = (p.Nj + 1) / 2;
    const int a = Na - 3, b = Nb - 3;
    auto cdiv = [](int x, int y) { return (x + y - 1) / y; };
    p.corner_gx = cdiv(b, kDense64JoinTileCols), p.corner_gy = cdiv(b, kDense64JoinTileRows);
    p.rows_gx = cdiv(a, kDense64JoinCrossCols), p.rows_gy = cdiv(b, kDense64JoinCrossRows);
    p.cols_gx = cdiv(b, kDense64JoinCrossCols), p.cols_gy = cdiv(a, kDense64JoinCrossRows);
    p.off_rows = 0;
    p.off_cols = 3 * (size_t)ld_dst;
    p.off_terms = 6 * (size_t)ld_dst;
    p.off_W = p.off_terms + 4 + 3 * (size_t)Nb;
    p.off_pose = p.off_W + 3 * (size_t)Nb;
    p.doubles = p.off_pose + 4;
    return p;
}
}  // namespace ekf
