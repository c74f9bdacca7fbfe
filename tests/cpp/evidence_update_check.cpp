// The bookkeeping of the scan evidence (ekf_dense64_evidence.hpp) as a stand-alone program: fixed counts through
// ekf::evidence_update, one line per landmark "i verdict logodds" (17 significant digits), then "ok".  Built plain and with
// -fsanitize=address,undefined by tests/test_dense64_evidence_host.py, which compares the lines with the Python restatement.
#include <cstdio>
#include <vector>

#include "../../ekf_slam_ml_amd/csrc/ekf_dense64_evidence.hpp"

int main() {
    // a deterministic family: every residue of (expected, agree, through) against min_beams = 3, both clamps met
    std::vector<int> e, a, t;
    std::vector<double> l;
    unsigned s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (int)((s >> 16) & 0x7fff); };
    for (int i = 0; i < 200; i++) {
        const int ex = next() % 12, ag = ex ? next() % (ex + 1) : 0, th = ex - ag ? next() % (ex - ag + 1) : 0;
        e.push_back(ex);
        a.push_back(ag);
        t.push_back(th);
        l.push_back(-4.5 + 0.045 * i);
    }
    e.push_back(2147483647); a.push_back(1073741824); t.push_back(1073741823); l.push_back(0.0);   // 2 a would overflow an int
    e.push_back(2147483647); a.push_back(0); t.push_back(2147483647); l.push_back(0.0);
    const int n = (int)e.size();
    std::vector<int> v(n, 7);
    ekf::evidence_update(n, e.data(), a.data(), t.data(), 3, 0.4, 0.85, -4.0, 4.0, l.data(), v.data());
    for (int i = 0; i < n; i++) std::printf("%d %d %.17g\n", i, v[i], l[i]);
    std::vector<double> l2(l);
    ekf::evidence_update(n, e.data(), a.data(), t.data(), 3, 0.4, 0.85, -4.0, 4.0, l2.data(), nullptr);   // verdict nullable
    for (int i = 0; i < n; i++)
        if (l2[i] < -4.0 || l2[i] > 4.0) return 1;
    std::puts("ok");
    return 0;
}
