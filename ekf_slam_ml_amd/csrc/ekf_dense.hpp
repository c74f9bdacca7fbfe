// ekf_dense.hpp -- the launchers of the dense handles' kernels: the MFMA GEMM of the dense covariance propagation, one
// template over the element type for the fp32 and the fp64 handle (ekf_dense.hip, kernels in ekf_dense_gemm.hpp), and every
// other kernel file of the fp64 handle (ekf_dense64_*.hip), one section each.  The limits of the fp64 calls (kDense64Max*)
// come from ekf_dense64_layout.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "ekf_dense64_layout.hpp"
#include "ekf_dense64_region.hpp"
#include "ekf_dense_split.hpp"   // kDenseTile = 128: ld must be a multiple of it

namespace ekf {
// ---- the GEMM of the propagation, E = float (v_mfma_f32_32x32x2_f32) or double (v_mfma_f64_16x16x4_f64); instantiated for
// these two in ekf_dense.hip.
// C[ld x ld] = A * B (+ Qadd), all row-major with zero padding up to ld.
// b_transposed: B is supplied as Bt[j][k] (i.e. C = A * Bt^T).
// n_rows (0 = ld): rows of C that are not padding; A's rows from there on are zero and C's were allocated zero.
template <class E>
void launch_dense_gemm(const E* A, const E* B, E* C, const E* Qadd, int ld, bool b_transposed, hipStream_t s, int n_rows = 0);
// how launch_dense_gemm cuts a product (ekf_dense_split.hpp): *tiles = ld / 128; n_big main tiles -- 256 x 128 in fp32,
// 128 x 128 in fp64 -- on the main kernel (k_gemm_big, whole rounds of resident workgroups); n_rem tiles of 128 x 128 -- the
// rest of the main-tile list and, in fp32, the bottom strip of an ld that is an odd multiple of 128 -- done as 4 * n_rem
// quarter tiles of 64 x 64 (k_gemm_tail) behind it
template <class E> void dense_gemm_split(int ld, int* tiles, int* n_big, int* n_rem);
// map [tiles][tiles] over the 128 x 128 blocks of C: 0 = computed by the main kernel, 1 = by the tail kernel (255 never)
template <class E> void dense_gemm_tile_map(int ld, unsigned char* map);
// raises the dynamic-LDS limit of the main kernel (49.4 KB per workgroup in fp32, 64.8 KiB in fp64)
template <class E> hipError_t dense_gemm_prepare();

// ---- fp64 dense measurement update for a general m x N Jacobian (ekf_dense64_correct.hip), on the same ld x ld Sigma:
//   T = H Sigma, U = Sigma H^T, S = T H^T + R, K = U S^-1, state += K nu, Sigma <- Sigma - K T, nis = nu^T S^-1 nu.
// How one correction of an N x N covariance is cut, and where its panels sit in the workspace (offsets in doubles).
struct Dense64CorrectPlan {
    int N, ld;
    int n_strips, n_chunks, tiles_per_chunk;   // panel pass: strips of 256 columns x chunks of 64-row tiles
    int n_sparts;                              // 128-column chunks of S = T H^T
    int upd_strips, upd_chunks, upd_blocks_per_chunk;   // update: strips of 128 columns x chunks of 16-row blocks
    size_t off_T, off_Ut, off_Kt, off_Tpart, off_Upart, off_Spart, off_Sinv, ws_doubles;
    int live;   // 0: N spans the handle; 1: N is a live dimension below it (dense64_live_plan) and indices >= N are off limits
};
Dense64CorrectPlan dense64_correct_plan(int N, int ld);
// The plan of the structured calls (the sparse corrections, the flush) at live dimension Na <= full.N on the same ld and
// the same workspace layout; `full` itself at Na == full.N.
Dense64CorrectPlan dense64_live_plan(const Dense64CorrectPlan& full, int Na);
hipError_t dense64_correct_prepare();   // raises the dynamic-LDS limits (panel pass: up to 99 KiB per workgroup at m > 48)
// The six launches of one correction on stream s.  Sigma: ld x ld with zero padding (kept); state: ld doubles;
// ws: pl.ws_doubles doubles; Hd: H as [m][ld] and Ht: H^T as [ld][m rounded up to 16], both zero padded; R: m x m; nu: m or NULL (state
// and *nis untouched); verdict: device word, 0 = applied, 1 = S singular or non-finite (then nothing was written to
// state or Sigma).
void launch_dense64_correct(const Dense64CorrectPlan& pl, double* Sigma, double* state, double* ws, const double* Hd,
                            const double* Ht, const double* R, const double* nu, int m, double* nis, int* verdict,
                            hipStream_t s);

// ---- fp64 batched scoring of J candidate measurements (ekf_dense64_score.hip), read-only on the same Sigma:
//   S_j = (H_j Sigma) H_j^T + R_j, nis_j = nu_j^T S_j^-1 nu_j, flag_j = S_j singular or not finite.
constexpr int kDense64ScoreGroup = 64;      // rows of stacked Jacobians per row group; candidates are packed whole
struct Dense64ScorePlan {
    Dense64CorrectPlan panels;   // strips / chunks of the pass over Sigma: those of the correction, a function of (N, ld)
    int cpg, n_groups;           // candidates per group = 64 / m, groups = ceil(J / cpg)
    int n_parts;                 // partial S blocks per candidate = n_chunks * n_strips
    size_t h_doubles;            // the stacked Jacobians on the device: [n_groups * 64][ld]
    size_t spart_doubles;        // the partial blocks: [n_parts][J][m * m]
};
Dense64ScorePlan dense64_score_plan(int N, int ld, int J, int m);
hipError_t dense64_score_prepare();   // raises the dynamic-LDS limits (panel pass 65 KiB at 64 rows, inversion 67 KiB)
// The three launches of one scoring call on stream s.  Hs: [n_groups * 64][ld], row g * 64 + q * m + r = row r of candidate
// g * cpg + q, columns N .. ld zero (rows without a candidate may hold anything); Spart: sp.spart_doubles doubles;
// R: [J][m][m] or [m][m] (r_shared); nu: [J][m] or NULL with nis NULL; nis [J] nullable; S_io [J][m][m]: workspace that
// holds the S_j on return; flag [J].
void launch_dense64_score(const Dense64ScorePlan& sp, const double* Sigma, const double* Hs, double* Spart,
                          const double* R, int r_shared, const double* nu, int J, int m, double* nis, double* S_io,
                          int* flag, hipStream_t s);

// ---- fp64 block-structured prediction (ekf_dense64_block.hip) on the same Sigma and state: F = identity with the r x r
// Jacobian Fr in [first, first + r)^2, Q = zero with Qr in the same square.  One launch of 1 + 2 ceil(N / 64) workgroups
// (the corner, the row panel and the column panel in strips of 64); touches nothing outside the block's rows and columns.
size_t dense64_block_lds_bytes(int r);   // dynamic LDS of the launch: one r x 64 tile, 32.5 KiB at r = 64
hipError_t dense64_block_prepare();      // nothing to raise at that size; kept so that every dense64 kernel file has one
// Fr: r x r row-major, Qr: r x r or NULL, dx: r or NULL (state untouched), all on the device; 1 <= r <= 64,
// 0 <= first, first + r <= N (the launcher does not check).
void launch_dense64_block(double* Sigma, double* state, const double* Fr, const double* Qr, const double* dx, int N,
                          int ld, int first, int r, hipStream_t s);

// ---- fp64 measurement update and scoring for a Jacobian with s listed non-zero columns (ekf_dense64_sparse.hip):
// H[:, cols[k]] = Hc[:, k], every dot product exactly s fused multiply-adds in ascending k of the list.  Eager, or
// deferred: p <= 64 pending rows of two panels [64][ld], Kp[q][i] = K[i][q] and Tq[q][j] = T[q][j], stand for
// Sigma_cur = Sigma - sum_{q < p} Kp[q]^T Tq[q]; the correction and the scoring read through them,
// x = fma(-Kp[q][row], Tq[q][col], x) in ascending q before the dot products, and Sigma is rewritten once per flush.
// raises the dynamic-LDS limits of both forms (gather 64.8 / 128.8 KiB, scoring up to 98.8 / 114.8 KiB)
hipError_t dense64_sparse_prepare();
// One launch: per candidate S_j = (Hc_j Sigma_cur[cols_j, cols_j]) Hc_j^T + R_j, flag_j, nis_j.  All pointers on the device:
// Kp, Tq and their row count p >= 0 (p = 0: the eager kernel on Sigma as it is, the panels not looked at), cols [J][s]
// (distinct, in [0, N): the launcher does not check), Hc [J][m][s], R [J][m][m] or [m][m] (r_shared), nu [J][m] or NULL
// with nis NULL, nis [J] nullable, S_out [J][m][m] nullable, flag [J], Sinv [64][64] nullable (the inverse of candidate 0
// when its flag is 0).
void launch_dense64_score_sparse(const double* Sigma, const double* Kp, const double* Tq, int p, const int* cols,
                                 const double* Hc, const double* R, int r_shared, const double* nu, int J, int m, int s,
                                 int ld, double* nis, double* S_out, int* flag, double* Sinv, hipStream_t st);
// Launches 5 and 6 of launch_dense64_correct (k_dc_gain, k_dc_update) on panels and an S^-1 already in ws.
void launch_dense64_correct_tail(const Dense64CorrectPlan& pl, double* Sigma, double* state, double* ws, const double* nu,
                                 int m, const int* verdict, hipStream_t s);
// The four launches of one sparse correction: the panel gather into ws (off_T, off_Ut), the scoring kernel with J = 1
// (S^-1 into off_Sinv, the verdict word, nis), then the gain and the update of the dense correction.
void launch_dense64_correct_sparse(const Dense64CorrectPlan& pl, double* Sigma, double* state, double* ws,
                                   const int* cols, const double* Hc, const double* R, const double* nu, int m, int s,
                                   double* nis, int* verdict, hipStream_t st);
// The first two of those launches alone (the eager gather, the scoring kernel with J = 1), with the summed S [m][m] written
// to S_out as well (nullable): what a caller with a gain and an update of its own needs (ekf_dense64_joseph.hip).
void launch_dense64_sparse_panels(const Dense64CorrectPlan& pl, const double* Sigma, double* ws, const int* cols,
                                  const double* Hc, const double* R, const double* nu, int m, int s, double* nis,
                                  double* S_out, int* verdict, hipStream_t st);
// Launch 5 of launch_dense64_correct (k_dc_gain) on U^T and S^-1 in ws, K^T written to Kt [m][ld] instead of ws.
void launch_dense64_gain(const Dense64CorrectPlan& pl, const double* ws, double* Kt, double* state, const double* nu, int m,
                         const int* verdict, hipStream_t s);
// The three launches of one deferred sparse correction, p + m <= 64, all on the deferred kernels (at p = 0 too): the gather
// through the pending rows (T into rows p .. p + m - 1 of Tq, U^T into ws), the scoring kernel with J = 1 (S^-1 into ws,
// the verdict word, nis), the gain (K^T into rows p .. p + m - 1 of Kp, state += K nu).  Sigma is not written; a set
// verdict leaves rows q < p and the state.
void launch_dense64_correct_deferred(const Dense64CorrectPlan& pl, const double* Sigma, double* state, double* ws,
                                     double* Kp, double* Tq, int p, const int* cols, const double* Hc, const double* R,
                                     const double* nu, int m, int s, double* nis, int* verdict, hipStream_t st);
// Launch 6 of launch_dense64_correct (k_dc_update) at rank p on the pending panels; zero: a device word that holds 0.
void launch_dense64_flush(const Dense64CorrectPlan& pl, double* Sigma, const double* Kp, const double* Tq, int p,
                          const int* zero, hipStream_t s);

// ---- the Joseph form of the sparse correction with per-state gain weights (ekf_dense64_joseph.hip; the definition is
// include/ekfslam.h's, ekf_dense64_correct_sparse_joseph): Sigma <- Sigma - K T - D K^T with K = diag(w) U S^-1 and
// D = U - K S, one read-modify-write pass of rank 2 m over tiles of kDense64JosephTileRows x kDense64JosephTileCols.
constexpr int kDense64JosephMaxM = 32;        // two stacked panels of m rows fit the 64-row panel stride
constexpr int kDense64JosephTileRows = 16;    // a wave's unit: one row block ...
constexpr int kDense64JosephTileCols = 128;   // ... of a workgroup's column strip
constexpr int kDense64JosephThreads = 256;
hipError_t dense64_joseph_prepare();   // raises the dynamic-LDS limit of the update (64 KiB at m = 32)
// Where the call keeps what is its own inside the workspace of the plan (the partial panels of the dense correction, which
// no sparse call uses): the weights [ld] and S [32 * 32] as doubles, then one byte per state (w != 0), per row block and
// per column strip (bit 0: some w != 0 among its live states, bit 1: some w == 0).
struct Dense64JosephWs { double *w, *S; unsigned char *state_on, *block, *strip; };
Dense64JosephWs dense64_joseph_ws(const Dense64CorrectPlan& pl, double* ws);
// The four launches: launch_dense64_sparse_panels, k_dj_gain, k_dj_update.  w: the weights on the device (the region of
// dense64_joseph_ws) or NULL for all 1; everything else as launch_dense64_correct_sparse, 1 <= m <= 32.
void launch_dense64_correct_sparse_joseph(const Dense64CorrectPlan& pl, double* Sigma, double* state, double* ws,
                                          const int* cols, const double* Hc, const double* R, const double* nu,
                                          const double* w, int m, int s, double* nis, int* verdict, hipStream_t st);

// ---- fp64 (re)initialisation of a block of states (ekf_dense64_init.hip) on the same Sigma and state: the block
// b = [first, first + r) becomes a function of the s listed states with Jacobian G (r x s): F = identity with F[b, b] = 0
// and F[b, cols] = G, Q = zero with W in the block's square.  One launch of 1 + 2 ceil(N / 64) workgroups (the corner, the
// row panel and the column panel in strips of 64); reads rows cols and columns cols outside b only (nothing at s = 0),
// writes the block's rows and columns only.
size_t dense64_init_lds_bytes(int r, int s);   // dynamic LDS of the launch: 64.8 KiB at r = s = 64, none at s = 0
hipError_t dense64_init_prepare();             // raises the dynamic-LDS limit to that
// cols [s] (distinct, in [0, N), none in b: the launcher does not check), G: r x s row-major, both unused at s = 0;
// W: r x r or NULL (no addition); xb: r or NULL (state untouched); all on the device.  1 <= r <= 64, 0 <= s <= 64.
void launch_dense64_init(double* Sigma, double* state, const int* cols, const double* G, const double* W,
                         const double* xb, int N, int ld, int first, int r, int s, hipStream_t st);
// out[a][c] = Sigma[rows[a]][cols[c]], nr * nc <= kDense64ReadMax, every index in [0, N) (not checked here)
void launch_dense64_read_block(const double* Sigma, const int* rows, const int* cols, double* out, int nr, int nc, int ld,
                               hipStream_t st);

// ---- the pending rows carried through propagate_block, init_block and the block readout (ekf_dense64_carry.hip): those
// calls are congruences Sigma <- A Sigma A^T + Q with A = identity except rows [first, first + r), so they run on Sigma in
// memory unchanged while every pending row v of both panels takes v[first + a] <- sum_k M[a][k] v[src[k]] (k ascending
// from +0, one fma per term).  M: r x s row-major on the device; src: s indices on the device, or NULL for the block itself
// (then s == r, in place); s = 0 writes +0.  One launch of ceil(2 p / 4) workgroups; nothing at p = 0.
void launch_dense64_panel_map(double* Kp, double* Tq, int p, const double* M, const int* src, int ld, int first, int r,
                              int s, hipStream_t st);
// launch_dense64_read_block against Sigma_cur: x = fma(-Kp[q][rows[a]], Tq[q][cols[c]], x) for q = 0 .. p - 1, p >= 1.
// live < N (the handle's live dimension): an entry with a row or column >= live is returned as stored, the panels unread there.
void launch_dense64_read_block_deferred(const double* Sigma, const double* Kp, const double* Tq, int p, const int* rows,
                                        const int* cols, double* out, int nr, int nc, int ld, int N, int live,
                                        hipStream_t st);

// ---- the exchange of two blocks of states (ekf_dense64_swap.hip) on the same Sigma and state: Sigma <- P Sigma P^T,
// state <- P state for the P that swaps [first_a, first_a + r) with [first_b, first_b + r).  A pure copy, one launch of
// 1 + 2 ceil(N / 64) workgroups (the 2 r x 2 r intersection with the state, the row panel and the column panel in strips of
// 64); touches nothing outside the two blocks' rows and columns, and nothing at an index >= N.  No LDS.
// 1 <= r <= 64, both blocks inside [0, N), |first_a - first_b| >= r (the launcher does not check); either order.
void launch_dense64_swap(double* Sigma, double* state, int N, int ld, int first_a, int first_b, int r, hipStream_t st);
// The same exchange on the pending rows carried through it: entries [first_a, +r) and [first_b, +r) of every row q < p of
// both panels.  One launch of ceil(2 p / 4) workgroups; nothing at p = 0.
void launch_dense64_panel_swap(double* Kp, double* Tq, int p, int ld, int first_a, int first_b, int r, hipStream_t st);

// ---- the reference's landmark model and decision rule on the handle's state (ekf_dense64_landmarks.hip): state is
// [theta, x, y, m1x, m1y, ...], candidate j of a call is landmark first_lm + j.
// One thread per candidate: cols [count][5] = {0, 1, 2, 3 + 2 i, 4 + 2 i}, Hc [count][2][5] (predicted_terms), nu [count][2]
// = z - zhat with the bearing raw (wrap = 0, the score's) or wrapped (wrap = 1, the correction's), R [2][2] = r_meas I;
// Hc and nu on 16-byte boundaries.  3 + 2 (first_lm + count) <= the state's length (the launcher does not check).
// pose [3]: (theta, x, y) the model is taken at -- `state` itself for calculate_maha_dis and data_association (:331-333), the
// snapshot of measurement() (:109-111) otherwise; the landmark's position always comes from `state`.
void launch_dense64_lm_terms(const double* state, const double* pose, double sx, double sy, int first_lm, int count,
                             int wrap, double r_meas, int* cols, double* Hc, double* R, double* nu, hipStream_t st);
// what k_dlm_decide leaves for the host: 32 bytes
enum : int { kDense64LmCorrect = 1, kDense64LmNew = 2 };
struct Dense64LmRecord {
    int win;          // the landmark to correct (== known for a new one), -1: the reading is dropped
    int kind;         // kDense64LmCorrect | kDense64LmNew
    double best;      // the winning score, gate_new when no candidate won
    double runner;    // the second-smallest score of the call and its candidate (+inf, INT_MAX with fewer than two)
    int runner_idx, pad;
};
static_assert(sizeof(Dense64LmRecord) == 32, "the decision record is one 32-byte copy");
// One workgroup: best = gate_new, win = known, the scores nis [count] (count = 0: none, nis unread) in ascending index
// with a strict <, NaNs skipped; win == known < n_max: a new landmark, xb [2] = initialize_landmark, W [2][2] = sigma0 I,
// the gate sees 0; gate < gate_update: corrected.  Independent of the launch geometry (ties resolve to the lower index).
void launch_dense64_lm_decide(const double* nis, int count, int known, int n_max, double gate_new, double gate_update,
                              double sigma0, const double* state, double sx, double sy, Dense64LmRecord* rec, double* W,
                              double* xb, hipStream_t st);
// state[0] = normalize_angle(state[0]) unless *verdict != 0 (the correction before it refused and wrote nothing)
void launch_dense64_lm_wrap(double* state, const int* verdict, hipStream_t st);

// ---- the landmark front end for a whole scan at once (ekf_dense64_joint.hip): all readings scored against one state, one
// assignment, one stacked correction.  xy [J][2]: the readings in device memory, on a 16-byte boundary.
// One thread per candidate: candidate j * count + i is reading j of xy [n_readings][2] against landmark first_lm + i, its
// operands exactly those launch_dense64_lm_terms (wrap = 0) writes for reading j alone, at the same place of a buffer cut
// for n_readings * count <= kDense64ScoreSparseMaxRows / 2 candidates.
void launch_dense64_joint_terms(const double* state, const double* pose, const double* xy, int n_readings, int first_lm,
                                int count, double r_meas, int* cols, double* Hc, double* R, double* nu, hipStream_t st);
// One workgroup per reading over nis [n_readings][count] (count = the known landmarks; 0: nis unread).  pre [b]: best and the
// runner-up as launch_dense64_lm_decide leaves them; kind = kDense64LmCorrect and win = the landmark for a MATCH (win < count
// and best < gate_update), kind = kDense64LmNew and win = count for a NEW reading (nothing under gate_new), kind = 0 and
// win = -1 for a DROP.
void launch_dense64_joint_argmin(const double* nis, int n_readings, int count, double gate_new, double gate_update,
                                 Dense64LmRecord* pre, hipStream_t st);
// One workgroup, J <= kDense64JointMaxReadings threads.  Of the MATCH readings that claim one landmark the smallest (best, j)
// keeps it, the others drop; the NEW readings take the slots known, known + 1, .. in ascending j while slot < n_max (win =
// the slot, kind = New | Correct when 0 < gate_update), beyond that they drop.  rec [J]: the final records; head [4] =
// {n_match, n_new, n_pairs, 0}; pair_lm, pair_j [n_pairs]: landmark and reading of every record with Correct, ascending j;
// xb [n_new][2] = initialize_landmark (:200-214) at state[0..2]; W_full = sigma0 I at r = 64 (written when n_new >= 32),
// W_last = sigma0 I at r = 2 (n_new % 32).
void launch_dense64_joint_resolve(const Dense64LmRecord* pre, int J, int known, int n_max, double gate_update, double sigma0,
                                  const double* state, const double* xy, int* head, Dense64LmRecord* rec, int* pair_lm,
                                  int* pair_j, double* xb, double* W_full, double* W_last, hipStream_t st);
// One workgroup: the stacked operands of V <= kDense64JointMaxPairs pairs (landmark lm [v], reading rj [v] of xy, or reading
// v when rj is NULL) from `state`: cols [3 + 2 V], Hc [2 V][3 + 2 V] (zero outside the pose columns and the pair's own two),
// R [2 V][2 V] = r_meas I, nu [2 V] with the bearing wrapped.  The landmarks distinct and inside the state (not checked).
void launch_dense64_joint_operands(const double* state, const double* xy, const int* lm, const int* rj, int V, double r_meas,
                                   int* cols, double* Hc, double* R, double* nu, hipStream_t st);

// ---- joint compatibility association (ekf_dense64_jcbb.hip; the search is ekf_dense64_jcbb.hpp's, the definitions are
// include/ekfslam.h's, ekf_dense64_jcbb_candidates).  The arrays are JcbbLayout's, cut for 32 readings of 4 candidates.
// One workgroup per reading over nis [n_readings][count] (count = 0: nis unread), reading j0 + b: the up to max_cand lowest
// (score, index) pairs below gate_ic in ascending order into cand_lm / cand_nis [j][4] (-1 / +inf beyond cand_count [j]),
// best [j] and is_new [j] as launch_dense64_joint_argmin defines best and NEW.
void launch_dense64_jcbb_select(const double* nis, int n_readings, int count, int j0, int max_cand, double gate_ic,
                                double gate_new, int* cand_count, int* cand_lm, double* cand_nis, double* best, int* is_new,
                                hipStream_t st);
// One workgroup: offset [J] (the exclusive scan of cand_count), head [0] = P, and per candidate p = offset [j] + rank:
// reading_of, lm_of and the operands cols [p][5], Hc [p][2][5], nu [p][2] (bearing raw) of launch_dense64_joint_terms.
void launch_dense64_jcbb_terms(const double* state, const double* xy, int J, const int* cand_count, const int* cand_lm,
                               int* head, int* offset, int* reading_of, int* lm_of, int* cols, double* Hc, double* nu,
                               hipStream_t st);
// W [P][P][2][2], P = head [0] <= p_cap (the grid is cut for p_cap): W[p][q] = Hc_p Sigma[cols_p, cols_q] Hc_q^T in the order
// of the sparse scoring kernel, + r_meas I where p == q.  A thread per block, a workgroup per kDense64JcbbTile^2 of them.
void launch_dense64_jcbb_cross(const double* Sigma, int ld, const int* head, const int* cols, const double* Hc, double r_meas,
                               int p_cap, double* W, hipStream_t st);

// ---- the reference's motion model and the top of its measurement() on the handle's state (ekf_dense64_model.hip).
// One thread: Fr [3][3] = eye + A, Qr [3][3] = q_pose I, upd [3] of prediction() (:67-96) for the heading state[0] and the
// twist (dtheta, dx); |dtheta| < straight_eps takes the straight branch.  Fr, Qr, upd: where propagate_block's operands go.
void launch_dense64_model_predict(const double* state, double dtheta, double dx, double q_pose, double straight_eps,
                                  double* Fr, double* Qr, double* upd, hipStream_t st);
// pose [3] = state[0..2] (:109-111)
void launch_dense64_model_snapshot(const double* state, double* pose, hipStream_t st);
// One thread per landmark: state[3 + 2 i], state[4 + 2 i] = the position reading i (sensor_xy [n_lm][2], on a 16-byte
// boundary) has from `pose` (:114-125), for every i < n_lm; 3 + 2 n_lm <= the state's length (the launcher does not check).
void launch_dense64_model_init(const double* pose, const double* sensor_xy, int n_lm, double* state, hipStream_t st);

// ---- circle fitting of one laser scan, shaped for latency (ekf_dense64_scan.hip): rigid2d::CircleFitting::
// approxCirclePositions on ranges [nb] in device memory.  ONE workgroup of four waves: clustering by ballots, one wave per
// cluster, every sum in an order that depends on the cluster's point count alone.  head [2] = {circles kept, clusters};
// centres [max_out][2], radii [max_out]: the first max_out circles in cluster order; all_out [clusters][4] = x, y, r,
// is_circle of every cluster.  7 nb doubles of dynamic LDS.  1 <= nb <= kDense64ScanMaxBeams, 1 <= max_out <=
// kDense64ScanMaxClusters (the launcher does not check).
void launch_dense64_scan_circles(const double* ranges, int nb, int max_out, int* head, double* centres, double* radii,
                                 double* all_out, hipStream_t st);

// ---- the coupling between the live corner and the tail (ekf_dense64_live.hip): over the two rectangles of an N x N Sigma
// with exactly one index >= Na, the number of entries != 0 and the largest absolute value.  One streaming launch, integer
// atomics only.  out: two 64-bit words on the device, zero before the launch: the count, and the bits of the maximum.
void launch_dense64_coupling(const double* Sigma, int N, int ld, int Na, unsigned long long* out, hipStream_t st);

// ---- all pairs of landmarks scored against each other (ekf_dense64_pairs.hip): d2(a, b), a < b < n_lm, is the nis of
// ekf_dense64_score_sparse for m = 2, s = 4, cols = {3 + 2a, 4 + 2a, 3 + 2b, 4 + 2b}, Hc = [[1, 0, -1, 0], [0, 1, 0, -1]],
// R = r_merge I, nu = x[a] - x[b], bit for bit; per landmark the partner with the smallest score (lowest index on a tie, a
// flagged pair never), and the counts of pairs below `gate` and of flagged pairs.  One read of Sigma's landmark corner:
// a workgroup per tile (A <= B) of kDense64PairsTile landmarks a side, then a fold of tiles + 1 records per landmark.
constexpr int kDense64PairsTile = 32;
constexpr int kDense64PairsThreads = 256;
// the workspace of a call, byte offsets: count (two 64-bit words, zero before the launch: below, flagged) | d2 [n_lm] |
// the per-tile records | nearest [n_lm]
struct Dense64PairsPlan {
    int n_lm, tiles;
    size_t off_count, off_d2, off_part_d2, off_part_idx, off_nearest, bytes;
};
Dense64PairsPlan dense64_pairs_plan(int n_lm);
// Two launches.  Reads Sigma and state below index 3 + 2 n_lm only (<= the dimension: the launcher does not check).
void launch_dense64_pairs(const Dense64PairsPlan& p, const double* Sigma, const double* state, int ld, double r_merge,
                          double gate, void* ws, hipStream_t st);
// One thread: the operands above for the pair (lo, hi) where the sparse correction reads them, with nu = x[hi] - x[lo]: the
// innovation of the reading 0 of x[lo] - x[hi], the exact negative of the score's nu (S and nis keep their bits).
void launch_dense64_pair_terms(const double* state, int lo, int hi, double r_merge, int* cols, double* Hc, double* R,
                               double* nu, hipStream_t st);

// ---- a laser scan cast against the handle's own map (ekf_dense64_evidence.hip; the definitions are include/ekfslam.h's,
// ekf_dense64_scan_evidence).  Three launches behind the tolerances: the landmarks within reach of the pose compacted in
// ascending index (one workgroup, ballots), a workgroup per kDense64EvidenceBeamTile beams that walks the candidates through
// LDS kDense64EvidenceLmChunk at a time and classes its beams, integer atomics for every count.
constexpr int kDense64EvidenceBeamTile = 64;
constexpr int kDense64EvidenceLmChunk = 128;
constexpr int kDense64EvidenceThreads = 64;
// the workspace of a call, byte offsets: report (4 ints) | the four counters [4][count] ints -- zero before the launches,
// zero_bytes from off_report -- | tol [count] | the candidates' indices [count] and offsets from the pose [count][2] |
// ranges, expected [kDense64ScanMaxBeams] doubles each | hit [kDense64ScanMaxBeams] ints | class [kDense64ScanMaxBeams] bytes
struct Dense64EvidencePlan {
    int first_lm, count;
    size_t off_report, off_counts, zero_bytes, off_tol, off_cand_idx, off_cand_xy, off_ranges, off_expected, off_hit,
        off_class, bytes;
};
Dense64EvidencePlan dense64_evidence_plan(int first_lm, int count);
// tol [at, at + n) = flag ? +Inf : tol_abs + kappa sqrt(max(S[j][0][0], 0)) for S [n][2][2], flag [n] as the sparse scoring
// kernel left them; S == nullptr: tol_abs.
void launch_dense64_evidence_tol(const Dense64EvidencePlan& p, int at, int n, const double* S, const int* flag,
                                 double tol_abs, double kappa, void* ws, hipStream_t st);
// The two launches of the cast; have_ranges = 0: the expected scan only.  Reads the state below 3 + 2 (first_lm + count).
void launch_dense64_evidence(const Dense64EvidencePlan& p, const double* state, int n_beams, double range_max,
                             double border_width, double tube_radius, double tol_abs, int have_ranges, void* ws,
                             hipStream_t st);

// ---- the health of the live corner and its exact symmetrisation (ekf_dense64_health.hip; the definitions of every figure
// are include/ekfslam.h's, ekf_dense64_health_report).  A workgroup per tile pair (A <= B) of kDense64HealthTile states a
// side: Sigma[A rows, B cols] along rows from memory, Sigma[B rows, A cols] along rows through an LDS transpose.
constexpr int kDense64HealthTile = 64;
constexpr int kDense64HealthThreads = 256;
// the result words of a call, 64-bit each, zero before the launch
enum {
    kDense64HealthNonfinite = 0,   // count (health)
    kDense64HealthAsym,            // count of pairs that differ in bits (health; symmetrize: the pairs written)
    kDense64HealthMinor,           // count (health)
    kDense64HealthDiagBad,         // count (health)
    kDense64HealthMaxBits,         // the bits of the largest |Sigma[i][j] - Sigma[j][i]| (both)
    kDense64HealthMaxLoc,          // i << 32 | j of it, all ones without a pair (health)
    kDense64HealthMinDiag,         // the bits of the smallest diagonal entry, +Inf without one (health)
    kDense64HealthMinDiagIdx,      // its index as a signed 64-bit number, -1 without one (health)
    kDense64HealthWords
};
// the workspace of a call, byte offsets: words | diag [tiles * 64] | one (max, loc) record per tile pair | one (value,
// index) record per 256 diagonal entries
struct Dense64HealthPlan {
    int Na, tiles, diag_groups;
    size_t pairs, off_words, off_diag, off_rec_max, off_rec_loc, off_drec_val, off_drec_idx, bytes;
};
Dense64HealthPlan dense64_health_plan(int Na);
// Three launches (the diagonal, the tile pairs, the fold); Sigma[0:Na, 0:Na] is read once (the diagonal twice), nothing of
// it is written.  Nothing at a row or column index >= Na is read (Na <= the dimension: the launcher does not check).
void launch_dense64_health(const Dense64HealthPlan& p, const double* Sigma, int ld, void* ws, hipStream_t st);
// One launch, in place: reads the corner once, writes the two entries of every pair i < j < Na that differ in bits.  Only
// the first kDense64HealthWords words of the workspace are used: [Asym] and [MaxBits].
void launch_dense64_symmetrize(const Dense64HealthPlan& p, double* Sigma, int ld, void* ws, hipStream_t st);

// ---- the Cholesky factor of the live corner and the forward substitution against it (ekf_dense64_factor.hip; the
// definitions are include/ekfslam.h's, ekf_dense64_factor_report).  A blocked right-looking factorisation, block side
// kDense64FactorNB, in a snapshot buffer of the handle's own: `rows` = Na rounded up to the block side, row stride
// ldf = rows + NB doubles, zero where the corner is not (so no tile of the snapshot is ragged), the lower triangle holds L,
// the last NB columns hold the NEGATED panel of the block column in flight -- the A operand of the trailing update, which
// is gemm_tile<double, BT> with C = Qadd = the trailing tile: A22 + (-L21) L21^T.
constexpr int kDense64FactorNB = 64;
constexpr int kDense64FactorThreads = 256;
constexpr int kDense64WhitenMaxRhs = 64;
// what the diagonal-block kernel leaves per block column; the host folds them in ascending block order
struct Dense64FactorRecord {
    double min_pivot, max_pivot;   // over the columns of the block that were factored; +Inf / 0.0 if none
    double fail_pivot;             // the pivot that ended the factorisation (bits), 0.0 without one
    int min_i;                     // column of min_pivot (lowest on ties), -1 if none
    int fail_index;                // the column whose pivot was not (finite and > 0), -1 without one
};
// the workspace of a call, byte offsets: the verdict word (0 until a pivot fails) | one record per block column | the
// diagonal of L [rows]
struct Dense64FactorPlan {
    int Na, blocks, rows, ldf;
    size_t factor_bytes, off_verdict, off_rec, off_diag, bytes;
};
Dense64FactorPlan dense64_factor_plan(int Na);
// 1 + 3 launches per block column (the last one: 1): the copy of the corner's lower triangle (masked element by element:
// nothing of Sigma at an index >= Na or above the diagonal is read, nothing of it is written), then per block column the
// diagonal-block factor (one workgroup), the panel solve by substitution (one workgroup per NB rows below) and the trailing
// update (one workgroup per NB x NB tile of the trailing lower triangle).  Every kernel behind the first reads the verdict
// word before its first store and does nothing when a pivot has failed.  The verdict word zero before the launch.
void launch_dense64_factor(const Dense64FactorPlan& p, const double* Sigma, int ld, double* factor, void* ws, hipStream_t st);
// Y = L^-1 B: rhs [2][kDense64WhitenMaxRhs][p.rows] -- first the working copy, row r = right-hand side r, zero beyond Na and
// in the rows not in use, then Y in the same shape (every entry written).  One launch per block column (every workgroup
// solves the diagonal block for all right-hand sides, the first one stores it into Y, the others take it out of their NB
// rows of the working copy), then d2 [kDense64WhitenMaxRhs] = the squared norms, a fixed fold.
void launch_dense64_whiten(const Dense64FactorPlan& p, const double* factor, double* rhs, double* d2, hipStream_t st);
// X = L^-T Y: work and X are [kDense64WhitenMaxRhs][p.rows], the working copy = Y as launch_dense64_whiten leaves it (a copy:
// it is consumed).  One launch per block column, descending (every workgroup solves the transposed diagonal block for all
// right-hand sides, the first one stores it into X, the others take it out of the NB entries of the working copy that
// belong to their block column).  Every entry of X is written, 0.0 from Na on.
void launch_dense64_back(const Dense64FactorPlan& p, const double* factor, double* work, double* X, hipStream_t st);
// X = Z L^T (+ state): Z and X are [kDense64WhitenMaxRhs][p.ldf] -- the snapshot's row stride, so that the three operands of
// the shared GEMM tile have one -- Z zero beyond Na and in the rows not in use; state (nullable) holds at least Na entries.
// One launch, a workgroup per NB states; columns [0, p.rows) of every row of X are written.
void launch_dense64_color(const Dense64FactorPlan& p, const double* factor, const double* Z, const double* state, double* X,
                          hipStream_t st);

// ---- the map in another frame (ekf_dense64_frame.hip; the definition is include/ekfslam.h's, ekf_dense64_map_congruence):
// Sigma <- J Sigma J^T on the live corner for J = blockdiag(1, G, ..., G) + [C | 0], in place, one pass over tiles of
// kDense64FrameTileRows x kDense64FrameTileCols whose origins sit on odd indices (3 + ...), and the state that goes with it.
constexpr int kDense64FrameTileRows = 64;
constexpr int kDense64FrameTileCols = 128;
constexpr int kDense64FrameThreads = 256;
constexpr int kDense64FrameFixed = 0, kDense64FrameRobot = 1;   // EKF_DENSE64_FRAME_FIXED, EKF_DENSE64_FRAME_ROBOT
// the workspace of a call, offsets in doubles: terms = G [4] | C [Na][3] (room for ld rows) | the new state [ld] | the old
// pose rows [3][ld] | the old pose columns, transposed [3][ld] | the panels A | C^T | (D Sigma_c)^T, [9][ld]
struct Dense64FramePlan {
    int Na, ld, pairs;   // pairs: index 0 and the (Na - 1) / 2 pairs (1, 2), (3, 4), ...
    size_t off_terms, off_state, off_rows, off_cols, off_panels, doubles;
};
Dense64FramePlan dense64_frame_plan(int Na, int ld);   // Na odd, >= 3 (the caller checks)
// One launch: terms and the new state (Na entries) into the workspace from the state as it is; the state is not written.
// FIXED: G = [c, -s, s, c] from the arguments, C is not written.  ROBOT: cos and sin of state[0] on the device; the
// arguments behind `ws` are ignored.
void launch_dense64_frame_state(const Dense64FramePlan& p, int mode, const double* state, double* ws, double dtheta, double c,
                                double s, double tx, double ty, hipStream_t st);
// Three launches on the terms that sit in the workspace (has_C: C is read, otherwise the rank-6 part is skipped): the
// snapshot and the panels, the pass over Sigma[3:Na, 3:Na], the new pose rows and columns.  Nothing at an index >= Na is
// read or written.
void launch_dense64_frame_congruence(const Dense64FramePlan& p, double* Sigma, double* ws, bool has_C, hipStream_t st);

// ---- map joining (ekf_dense64_join.hip; the definition is include/ekfslam.h's, ekf_dense64_join_congruence; the plan and
// the workspace are ekf_dense64_layout.hpp's Dense64JoinPlan).  Everything runs on the one stream given: the destination's.
// One launch: cos and sin of state_dst[0] on the device, G and E into the terms, the composed pose into the staging slot
// (ws + off_pose; state_dst[0 .. 2] is not written), the source's landmarks in the destination's frame into state_dst[Na ...].
void launch_dense64_join_state(const Dense64JoinPlan& p, double* state_dst, const double* state_src, double* ws, hipStream_t st);
// Up to five launches on the terms that sit in the workspace: the snapshot and W, the pass over the source's Sigma[3:Nb, 3:Nb]
// (Nb > 3), the two rectangles (Na > 3 and Nb > 3), the new pose rows and columns.  The source is read only; of the
// destination nothing inside [3, Na) x [3, Na) and nothing at an index >= Na + Nb - 3 is read or written.
void launch_dense64_join_congruence(const Dense64JoinPlan& p, double* Sigma_dst, const double* Sigma_src, double* ws,
                                    hipStream_t st);

// ---- a map or a submap copied into a second handle (ekf_dense64_extract.hip; the definition is include/ekfslam.h's,
// ekf_dense64_extract_map): Sigma_dst[i][j] = Sigma_src[iota(i)][iota(j)], x_dst[i] = x_src[iota(i)] over [0, Nd), bits kept,
// iota: 0, 1, 2 -> 0, 1, 2 and 3 + 2 t + c -> 3 + 2 keep[t] + c.  Everything runs on the one stream given: the destination's.
constexpr int kDense64ExtractTileRows = 64;    // the hot pass: tiles of the DESTINATION's Sigma[3:Nd, 3:Nd], origins on odd indices
constexpr int kDense64ExtractTileCols = 128;
constexpr int kDense64ExtractThreads = 256;
// the workspace of a call (from the destination's ledger), offsets in ints: keep [k], zeros up to 64 corner_gx | run [corner_gx], run[b] != 0 where
// the landmarks of column tile b are a contiguous ascending run of the source (keep[64 b + l] = keep[64 b] + l)
struct Dense64ExtractPlan {
    int Nb, Nd, k, ld_src, ld_dst;   // Nd = 3 + 2 k
    int corner_gx, corner_gy;        // k_ex_corner's grid (0 x 0 at k = 0: not launched)
    int panel_cols;                  // a carried pending row is written on [0, panel_cols): Nd rounded up to kDenseTile, at most ld_dst
    size_t off_keep, off_run, ints;
};
inline Dense64ExtractPlan dense64_extract_plan(int Nb, int ld_src, int k, int ld_dst) {
    Dense64ExtractPlan p{};
    p.Nb = Nb, p.Nd = 3 + 2 * k, p.k = k, p.ld_src = ld_src, p.ld_dst = ld_dst;
    p.corner_gx = (2 * k + kDense64ExtractTileCols - 1) / kDense64ExtractTileCols;
    p.corner_gy = (2 * k + kDense64ExtractTileRows - 1) / kDense64ExtractTileRows;
    const int up = (p.Nd + kDenseTile - 1) / kDenseTile * kDenseTile;
    p.panel_cols = up < ld_dst ? up : ld_dst;
    p.off_keep = 0;
    p.off_run = (size_t)p.corner_gx * (kDense64ExtractTileCols / 2);   // (the list padded with zeros to whole column tiles)
    p.ints = p.off_run + (size_t)p.corner_gx + 4;                      // (never empty)
    return p;
}
// Two launches: the pass over the destination's Sigma[3:Nd, 3:Nd] (k > 0), and the pose rows and columns, the 3 x 3 corner
// and the Nd states.  ws: the list and the flags as the plan lays them out.  The source is read only and nothing of it at an
// index >= Nb is read (every keep[t] < (Nb - 3) / 2: the caller checks); nothing of the destination at an index >= Nd is
// read or written.
void launch_dense64_extract(const Dense64ExtractPlan& p, double* Sigma_dst, double* state_dst, const double* Sigma_src,
                            const double* state_src, const int* ws, hipStream_t st);
// One launch (none at rows = 0): the first `rows` rows of the source's pending panels through the same index map into the
// destination's, zero on [Nd, panel_cols).
void launch_dense64_extract_panels(const Dense64ExtractPlan& p, double* K_dst, double* T_dst, const double* K_src,
                                   const double* T_src, int rows, const int* ws, hipStream_t st);

// ---- a local region (ekf_dense64_region.hip; plan and layout in ekf_dense64_region.hpp, the definition is
// include/ekfslam.h's, ekf_dense64_region_begin): the accumulators Phi, Psi, theta of the compressed filter in `acc`
// (Dense64RegionPlan::acc_bytes), the two panels of the global update in `scratch` (scratch_bytes).
hipError_t dense64_region_prepare();   // raises the dynamic-LDS limit of the Sigma_bb product (64.8 KiB)
// One launch: Phi = I, Psi = 0, theta = 0.
void launch_dense64_region_reset(const Dense64RegionPlan& p, void* acc, hipStream_t st);
// The two launches behind a sparse correction of the live corner: the panels W = Hc Phi[cols, :], Z = S^-1 W and
// theta += Z^T nu, then Phi -= K W and Psi += W^T Z.  Kt [m][ldk] = K^T, Sinv [64][64], cols, Hc, nu (nullable) and the
// verdict word are the live call's own, on the device; a set verdict leaves everything as it was.
void launch_dense64_region_correct(const Dense64RegionPlan& p, void* acc, const double* Kt, int ldk, const double* Sinv,
                                   const int* cols, const double* Hc, const double* nu, int m, int s, const int* verdict,
                                   hipStream_t st);
// One launch: Phi[first .. first + r, :] <- M Phi[src, :], M r x s row-major on the device; src: s indices on the device,
// or NULL for the block itself (s == r, in place); s = 0 writes +0.
void launch_dense64_region_rowmap(const Dense64RegionPlan& p, void* acc, const double* M, const int* src, int first, int r,
                                  int s, hipStream_t st);
// The six launches of the global update, in the order the algebra needs (the first three read Sigma0_ab and Sigma0_ba):
// x_b, Y and V, Sigma_bb on the MFMA tile, Sigma_ba through the scratch, Sigma_ab.  Nothing with a row and a column index
// below Na is read or written; the padding of Sigma and of the state is neither.
void launch_dense64_region_end(const Dense64RegionPlan& p, double* Sigma, double* state, const void* acc, void* scratch,
                               hipStream_t st);

// ---- what observing each landmark would gain (ekf_dense64_value.hip; the definitions of every figure are
// include/ekfslam.h's, ekf_dense64_value_operands): for `count` landmarks from first_lm on, with U = Sigma H^T over the live
// corner, G = U^T U (all rows) and P = U^T U (rows 0 .. 2) in ONE read of Sigma[0:Na, 0:Na] along rows, S by the sparse
// scoring's own launch, then the trace drops tr(S^-1 G), tr(S^-1 P), det S and the three winners.
constexpr int kDense64ValueTileRows = 128;   // rows of Sigma a workgroup of the pass sums, in ascending order
constexpr int kDense64ValueTileLm = 128;     // landmarks of a workgroup of the pass: one per lane
constexpr int kDense64ValueThreads = 128;
// what the call leaves for the host; the layout of ekf_dense64_value_best (ekfslam.h)
struct Dense64ValueBest {
    int i_trace, i_pose, i_det, reserved;
    double v_trace, v_pose, v_det;
};
// the workspace of a call, byte offsets: Hc [count][2][5] | R [4] | S [count][4] | dtrace, dpose, detS [count] each | best |
// the records [row_tiles][6][count] | cols [count][5] | flag [count] | in_view [count]
struct Dense64ValuePlan {
    int Na, first_lm, count, row_tiles, lm_tiles;
    size_t off_Hc, off_R, off_S, off_dtrace, off_dpose, off_det, off_best, off_rec, off_cols, off_flag, off_view, bytes;
};
Dense64ValuePlan dense64_value_plan(int Na, int first_lm, int count);
// One launch, the model call's: Hc (measurement_terms of ekf_kernels.hpp on the state's own pose and landmarks), cols, the
// shared R = r_meas I and in_view = (predicted range <= range_max), or 1 when range_max <= 0.
void launch_dense64_value_terms(const Dense64ValuePlan& p, const double* state, double r_meas, double range_max, void* ws,
                                hipStream_t st);
// One launch, the operands call's: cols alone (Hc, R and in_view came up from the caller).
void launch_dense64_value_cols(const Dense64ValuePlan& p, void* ws, hipStream_t st);
// Four launches on operands that sit in ws: the sparse scoring (S, flag; eager: nothing may be pending), the pass over
// the corner, the fold per landmark, the winners.  Nothing at a row or column index >= Na is read (3 + 2 (first_lm +
// count) <= Na <= the dimension: the launcher does not check).  Sigma is not written.
void launch_dense64_value(const Dense64ValuePlan& p, const double* Sigma, int ld, void* ws, hipStream_t st);
}  // namespace ekf
