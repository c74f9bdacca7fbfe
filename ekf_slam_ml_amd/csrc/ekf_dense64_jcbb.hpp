// ekf_dense64_jcbb.hpp -- the host half of the joint compatibility association (Neira & Tardos, 2001) of the dense fp64
// handle: a bounded branch and bound over the candidates ekf_dense64_jcbb.hip selected and the cross blocks it computed.
// Nothing from HIP and header-only: ekf_capi_dense64.hip calls it behind the one synchronisation of the device half,
// tests/cpp/jcbb_search_check.cpp on a CPU.  The search is sequential, O(k^2) per node on at most 512 KB; the device part
// is whatever touches Sigma.
//   ORDER      depth first over the readings in ascending j; at reading j its candidates in ascending rank (a landmark the
//              hypothesis uses already is skipped), then the branch "j unpaired".  Every call of visit() is one node.
//   ACCEPT     an extension to k pairings only when its joint d2 < gate_joint[k - 1]
//   INCUMBENT  starts as "nothing paired" (0 pairings, d2 = 0); a leaf replaces it when it has more pairings, or as many and
//              a smaller d2 (strictly: the first found stands).  A node is pruned when pairings so far + readings from j on
//              that have a candidate < the incumbent's pairings.
//   D2         by an incremental Cholesky factor along the current path: one 64 x 64 L and one z, rows past the current
//              depth dead.  Pair number m of the path (candidate p) owns rows 2 m, 2 m + 1; Wfull[r][c] for an earlier pair's
//              column is W[p_new][p_old] (the lower triangle only; R sits in the diagonal blocks).  Per new row r, columns c
//              ascending, every product rounded and subtracted in turn, t ascending:
//                v = Wfull[r][c];  v = v - L[r][t] L[c][t]  (t < c);  L[r][c] = v / L[c][c]
//                d = Wfull[r][r];  d = d - L[r][t] L[r][t]  (t < r);  not (finite and > 0): the extension is incompatible
//                L[r][r] = sqrt(d);  s = nu[r];  s = s - L[r][t] z[t]  (t < r);  z[r] = s / L[r][r];  d2 = d2 + z[r] z[r]
//              This order is part of the contract (the library is built with -ffp-contract=off).
//   BUDGET     at most max_nodes nodes; when they run out the incumbent stands and exhausted = 1.  A function of its inputs.
#pragma once
#include <cmath>

namespace ekf {

constexpr int kJcbbMaxReadings = 32;
constexpr int kJcbbMaxCand = 4;
constexpr int kJcbbMaxP = kJcbbMaxReadings * kJcbbMaxCand;   // 128 candidates, W <= 256 x 256
constexpr long long kJcbbMaxNodes = 1LL << 22;

struct JcbbResult {
    int n_pairs;
    int exhausted;
    long long nodes;
    double d2;
};

// reading_of [P] ascending (the candidates in (j, rank) order), lm_of [P], W [2P][2P] row-major, nu [2P], gate_joint [J];
// assign [J]: the candidate of each reading, -1 unpaired.  The arguments are the caller's to check.
class JcbbSearch {
public:
    JcbbSearch(int J, int P, const int* reading_of, const int* lm_of, const double* W, const double* nu,
               const double* gate_joint, long long max_nodes)
        : J_(J), P_(P), lm_of_(lm_of), W_(W), nu_(nu), gate_(gate_joint), max_nodes_(max_nodes) {
        for (int j = 0; j <= J; j++) first_[j] = 0;
        for (int p = 0; p < P; p++) first_[reading_of[p] + 1]++;
        for (int j = 0; j < J; j++) first_[j + 1] += first_[j];
        to_come_[J] = 0;
        for (int j = J - 1; j >= 0; j--) to_come_[j] = to_come_[j + 1] + (first_[j + 1] > first_[j] ? 1 : 0);
    }
    JcbbResult run(int* assign) {
        for (int j = 0; j < J_; j++) cur_[j] = best_[j] = -1;
        best_pairs_ = 0;
        best_d2_ = 0.0;
        nodes_ = 0;
        exhausted_ = 0;
        visit(0, 0, 0.0);
        for (int j = 0; j < J_; j++) assign[j] = best_[j];
        return {best_pairs_, exhausted_, nodes_, best_d2_};
    }

private:
    bool used(int lm, int m) const {
        for (int i = 0; i < m; i++)
            if (lm_of_[path_[i]] == lm) return true;
        return false;
    }
    // pair number m of the path becomes candidate p: rows 2 m and 2 m + 1 of L and z
    bool extend(int m, int p, double& d2) {
        const int n = 2 * P_;
        for (int a = 0; a < 2; a++) {
            const int r = 2 * m + a;
            const double* wrow = W_ + (size_t)(2 * p + a) * n;
            double* Lr = L_[r];
            for (int c = 0; c < r; c++) {
                const int mc = c >> 1;
                double v = wrow[2 * (mc == m ? p : path_[mc]) + (c & 1)];
                const double* Lc = L_[c];
                for (int t = 0; t < c; t++) v = v - Lr[t] * Lc[t];
                Lr[c] = v / Lc[c];
            }
            double d = wrow[2 * p + a];
            for (int t = 0; t < r; t++) d = d - Lr[t] * Lr[t];
            if (!(std::isfinite(d) && d > 0.0)) return false;
            Lr[r] = std::sqrt(d);
            double s = nu_[2 * p + a];
            for (int t = 0; t < r; t++) s = s - Lr[t] * z_[t];
            z_[r] = s / Lr[r];
            d2 = d2 + z_[r] * z_[r];
        }
        return true;
    }
    void visit(int j, int m, double d2) {
        if (nodes_ >= max_nodes_) {
            exhausted_ = 1;
            return;
        }
        nodes_++;
        if (j == J_) {
            if (m > best_pairs_ || (m == best_pairs_ && d2 < best_d2_)) {
                best_pairs_ = m;
                best_d2_ = d2;
                for (int i = 0; i < J_; i++) best_[i] = cur_[i];
            }
            return;
        }
        if (m + to_come_[j] < best_pairs_) return;
        for (int p = first_[j]; p < first_[j + 1]; p++) {
            if (used(lm_of_[p], m)) continue;
            double e = d2;
            if (!extend(m, p, e) || !(e < gate_[m])) continue;
            path_[m] = p;
            cur_[j] = p;
            visit(j + 1, m + 1, e);
            cur_[j] = -1;
            if (exhausted_) return;
        }
        visit(j + 1, m, d2);
    }

    int J_, P_;
    const int* lm_of_;
    const double *W_, *nu_, *gate_;
    long long max_nodes_, nodes_ = 0;
    int first_[kJcbbMaxReadings + 1], to_come_[kJcbbMaxReadings + 1];
    int path_[kJcbbMaxReadings], cur_[kJcbbMaxReadings], best_[kJcbbMaxReadings];
    int best_pairs_ = 0, exhausted_ = 0;
    double best_d2_ = 0.0;
    double L_[2 * kJcbbMaxReadings][2 * kJcbbMaxReadings], z_[2 * kJcbbMaxReadings];
};

// 0 when the arguments are a search's: 1 <= J <= 32, 0 <= P <= 128, reading_of ascending in [0, J) with at most 4 candidates
// a reading, lm_of >= 0, every gate finite and > 0, 1 <= max_nodes <= 2^22
inline int jcbb_arguments_bad(int J, int P, const int* reading_of, const int* lm_of, const double* gate_joint,
                              long long max_nodes) {
    if (J < 1 || J > kJcbbMaxReadings || P < 0 || P > kJcbbMaxP || max_nodes < 1 || max_nodes > kJcbbMaxNodes) return 1;
    int run = 0;
    for (int p = 0; p < P; p++) {
        if (reading_of[p] < 0 || reading_of[p] >= J || lm_of[p] < 0) return 1;
        if (p > 0 && reading_of[p] < reading_of[p - 1]) return 1;
        run = (p > 0 && reading_of[p] == reading_of[p - 1]) ? run + 1 : 1;
        if (run > kJcbbMaxCand) return 1;
    }
    for (int k = 0; k < J; k++)
        if (!(std::isfinite(gate_joint[k]) && gate_joint[k] > 0.0)) return 1;
    return 0;
}

}  // namespace ekf
