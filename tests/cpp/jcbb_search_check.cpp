// jcbb_search_check.cpp -- the search of ekf_dense64_jcbb.hpp on a CPU, a plain C++17 program with its own main (built by
// tests/test_dense64_jcbb_host.py, plain and with -fsanitize=address,undefined).  Two inputs, written out as data:
//   budget   8 readings x 4 mutually compatible candidates on distinct landmarks, W = I, the innovation growing with the rank;
//            50 nodes end with exhausted = 1 and every reading at its rank 0
//   worst    P = 128: 32 readings x 4 candidates, W = I + 1/4 (every pairing correlated with every other: the factor fills
//            all 64 rows), loose gates; 2^16 nodes end exhausted with 32 pairings, and a second run repeats the first
// Prints one line per case: name n_pairs exhausted nodes d2 (17 digits) assign...; exit status 0 when the checks hold.
#include <cstdio>
#include <vector>

#include "../../ekf_slam_ml_amd/csrc/ekf_dense64_jcbb.hpp"

namespace {

struct Case {
    int J, C;
    std::vector<int> reading_of, lm_of;
    std::vector<double> W, nu, gates;
};

Case make(int J, int C, double off_diag, double gate) {
    Case c{J, C, {}, {}, {}, {}, {}};
    const int P = J * C, n = 2 * P;
    c.W.assign((size_t)n * n, off_diag);
    for (int r = 0; r < n; r++) c.W[(size_t)r * n + r] = 1.0 + off_diag;
    c.nu.assign(n, 0.0);
    for (int p = 0; p < P; p++) {
        c.reading_of.push_back(p / C);
        c.lm_of.push_back(p);
        c.nu[2 * p] = 0.125 * (1 + p % C);
    }
    for (int k = 0; k < J; k++) c.gates.push_back((k + 1) * gate);
    return c;
}

ekf::JcbbResult run(const char* name, const Case& c, long long max_nodes, std::vector<int>& assign) {
    const int P = c.J * c.C;
    assign.assign(c.J, -2);
    if (ekf::jcbb_arguments_bad(c.J, P, c.reading_of.data(), c.lm_of.data(), c.gates.data(), max_nodes)) {
        std::printf("%s: arguments refused\n", name);
        return {-1, 0, 0, 0.0};
    }
    ekf::JcbbSearch s(c.J, P, c.reading_of.data(), c.lm_of.data(), c.W.data(), c.nu.data(), c.gates.data(), max_nodes);
    const ekf::JcbbResult r = s.run(assign.data());
    std::printf("%s %d %d %lld %.17g", name, r.n_pairs, r.exhausted, r.nodes, r.d2);
    for (int a : assign) std::printf(" %d", a);
    std::printf("\n");
    return r;
}

}  // namespace

int main() {
    int bad = 0;
    std::vector<int> a, b;
    const Case budget = make(8, 4, 0.0, 100.0);
    ekf::JcbbResult r = run("budget", budget, 50, a);
    bad += !(r.n_pairs == 8 && r.exhausted == 1 && r.nodes == 50 && r.d2 == 8 * 0.125 * 0.125);
    for (int j = 0; j < 8; j++) bad += a[j] != 4 * j;
    const Case worst = make(32, 4, 0.25, 1000.0);
    r = run("worst", worst, 1LL << 16, a);
    const ekf::JcbbResult again = run("worst", worst, 1LL << 16, b);
    bad += !(r.n_pairs == 32 && r.exhausted == 1 && r.nodes == (1LL << 16));
    bad += !(again.n_pairs == r.n_pairs && again.nodes == r.nodes && again.d2 == r.d2 && a == b);
    r = run("one", worst, 1, a);   // a budget of one node: the incumbent "nothing paired" stands
    bad += !(r.n_pairs == 0 && r.exhausted == 1 && r.nodes == 1 && r.d2 == 0.0);
    for (int j = 0; j < 32; j++) bad += a[j] != -1;
    // what the entry point refuses: too many candidates for a reading, a reading out of order, a gate that is not a gate
    Case c = make(2, 4, 0.0, 1.0);
    c.reading_of[4] = 0;
    bad += !ekf::jcbb_arguments_bad(2, 8, c.reading_of.data(), c.lm_of.data(), c.gates.data(), 10);
    c = make(2, 2, 0.0, 1.0);
    c.gates[1] = 0.0;
    bad += !ekf::jcbb_arguments_bad(2, 4, c.reading_of.data(), c.lm_of.data(), c.gates.data(), 10);
    bad += !ekf::jcbb_arguments_bad(33, 0, nullptr, nullptr, c.gates.data(), 10);
    std::printf(bad ? "FAILED %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
