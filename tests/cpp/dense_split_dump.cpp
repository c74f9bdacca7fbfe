// dense_split_dump.cpp -- walks the tile lists of the dense propagation (ekf_dense_split.hpp) for both element types and
// every ld = 128 k, k = 1 .. 80, for tests/test_dense_split_host.py.  Per (type, ld) three lines:
//   <f32|f64> <ld> split <tiles_m> <tiles_n> <n_big> <rem_big> <bottom> <n_small> <xcd_remap is a permutation of [0, n_big)>
//   <f32|f64> <ld> owners <per 128 x 128 block of C, row-major: main-kernel owners * 16 + tail-kernel owners, a hex digit pair>
//   <f32|f64> <ld> map <dense_tile_map of the same blocks, two hex digits each>
// A tile that reaches outside C is reported as `outside` instead.  Needs no HIP: g++ -std=c++17 -I ekf_slam_ml_amd/csrc.
#include <cstdio>
#include <vector>

#include "ekf_dense_split.hpp"

template <class E>
static void dump(const char* name) {
    constexpr int PER = ekf::kDenseMainRows<E> / ekf::kDenseTile;
    for (int k = 1; k <= 80; k++) {
        const int ld = ekf::kDenseTile * k;
        const ekf::DenseSplit sp = ekf::make_split<E>(ld);
        const int t = sp.tiles_n;
        std::vector<unsigned char> own(t * t, 0), map(t * t, 0), seen(sp.n_big, 0);
        bool perm = true, outside = t != k;
        for (int id = 0; id < sp.n_big; id++) {
            const int r = ekf::xcd_remap(id, sp.n_big);
            if (r < 0 || r >= sp.n_big || seen[r]++) { perm = false; continue; }
            int tm, tn;
            ekf::big_tile_of(r, sp.tiles_m, sp.tiles_n, tm, tn);
            if (tm < 0 || tn < 0 || PER * (tm + 1) > t || tn >= t) { outside = true; continue; }
            for (int h = 0; h < PER; h++) own[(PER * tm + h) * t + tn] += 16;
        }
        for (int q = 0; q < sp.n_small; q++) {
            int r0, c0;
            ekf::small_tile_origin<E>(sp, q, r0, c0);
            if (r0 < 0 || c0 < 0 || r0 % ekf::kDenseTile || c0 % ekf::kDenseTile || r0 >= ld || c0 >= ld) { outside = true; continue; }
            own[(r0 / ekf::kDenseTile) * t + c0 / ekf::kDenseTile] += 1;
        }
        std::printf("%s %d split %d %d %d %d %d %d %d\n", name, ld, sp.tiles_m, sp.tiles_n, sp.n_big, sp.rem_big, sp.bottom,
                    sp.n_small, perm ? 1 : 0);
        if (outside) {
            std::printf("%s %d outside\n", name, ld);
            continue;
        }
        ekf::dense_tile_map<E>(sp, map.data());
        std::printf("%s %d owners ", name, ld);
        for (unsigned char c : own) std::printf("%02x", c);
        std::printf("\n%s %d map ", name, ld);
        for (unsigned char c : map) std::printf("%02x", c);
        std::printf("\n");
    }
}

int main() {
    dump<float>("f32");
    dump<double>("f64");
    return 0;
}
