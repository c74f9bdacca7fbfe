// dense64_scan_layout_dump.cpp -- prints the layout of the dense handle's scan buffer (ekf_dense64_layout.hpp: scan_layout)
// as `key value` lines (bytes), and the two limits it is cut for, for tests/test_dense64_scan_host.py.  Needs no HIP:
// g++ -std=c++17 -I ekf_slam_ml_amd/csrc.
#include <cstdio>

#include "ekf_dense64_layout.hpp"

int main() {
    const ekf::d64::ScanLayout l = ekf::d64::scan_layout();
    std::printf("ranges %zu\nhead %zu\ncentres %zu\nradii %zu\nall %zu\nbytes %zu\nrecord_bytes %zu\n", l.ranges, l.head,
                l.centres, l.radii, l.all, l.bytes, l.record_bytes);
    std::printf("max_beams %d\nmax_clusters %d\n", ekf::kDense64ScanMaxBeams, ekf::kDense64ScanMaxClusters);
    return 0;
}
