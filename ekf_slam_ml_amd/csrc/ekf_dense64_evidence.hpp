// ekf_dense64_evidence.hpp -- the host half of the scan evidence of the dense fp64 handle: what the per-landmark counts of
// ekf_dense64_scan_evidence (ekf_dense64_evidence.hip) do to a caller-kept array of log-odds.  Nothing from HIP and
// header-only: ekf_capi_dense64.hip calls it behind ekf_dense64_evidence_update, tests/cpp/evidence_update_check.cpp on a
// CPU.  Per landmark i, in ascending i, with e = n_expected[i], a = n_agree[i], t = n_through[i]:
//   e < min_beams      too few beams to say anything: verdict 0, the log-odds untouched apart from the clamp
//   2 a >= e           a HIT:  l = l + w_hit,  verdict +1      (at least half of the beams stopped on the landmark)
//   2 t >  e           a MISS: l = l - w_miss, verdict -1      (more than half went through where it should stand)
//   otherwise          verdict 0 (mostly short beams: something unmapped is in the way)
// and then l = min(max(l, l_min), l_max).  a + t <= e, so a hit and a miss exclude each other.  The decisions are integer
// comparisons (in 64 bits: 2 a cannot overflow), the sums plain fp64, one rounding each.
#pragma once

namespace ekf {

// the arrays [count]; verdict nullable.  The arguments are the caller's to check.
inline void evidence_update(int count, const int* n_expected, const int* n_agree, const int* n_through, int min_beams,
                            double w_hit, double w_miss, double l_min, double l_max, double* logodds, int* verdict) {
    for (int i = 0; i < count; i++) {
        const long long e = n_expected[i], a = n_agree[i], t = n_through[i];
        int v = 0;
        double l = logodds[i];
        if (e >= min_beams) {
            if (2 * a >= e) {
                l = l + w_hit;
                v = 1;
            } else if (2 * t > e) {
                l = l - w_miss;
                v = -1;
            }
        }
        if (l < l_min) l = l_min;
        if (l > l_max) l = l_max;
        logodds[i] = l;
        if (verdict) verdict[i] = v;
    }
}

}  // namespace ekf
