// dense64_layout_dump.cpp -- prints every offset and size of every layout of ekf_dense64_layout.hpp as `name key value`
// lines (bytes), for tests/test_dense64_layout_host.py.  Needs no HIP: g++ -std=c++17 -I ekf_slam_ml_amd/csrc.
#include <cstdio>
#include <initializer_list>
#include <string>
#include <utility>

#include "ekf_dense64_layout.hpp"

using namespace ekf::d64;

static void dump(const std::string& name, std::initializer_list<std::pair<const char*, size_t>> rows) {
    for (const auto& r : rows) std::printf("%s %s %zu\n", name.c_str(), r.first, r.second);
}

int main() {
    for (int ld : {128, 256, 10112}) {
        const std::string at = "@" + std::to_string(ld);
        const CorrInLayout c = corr_in_layout(ld);
        dump("corr_in" + at, {{"H", c.H}, {"Ht", c.Ht}, {"R", c.R}, {"nu", c.nu}, {"bytes", c.bytes}});
        const CorrSparseLayout cs = corr_sparse_layout(ld);
        dump("corr_sparse" + at, {{"Hc", cs.Hc}, {"cols", cs.cols}, {"R", cs.R}, {"nu", cs.nu}, {"bytes", cs.bytes}});
        const PendLayout p = pend_layout(ld);
        dump("pend" + at, {{"K", p.K}, {"T", p.T}, {"zero", p.zero}, {"bytes", p.bytes}});
    }
    const CorrOutLayout co = corr_out_layout();
    dump("corr_out", {{"nis", co.nis}, {"verdict", co.verdict}, {"bytes", co.bytes}});
    const ScSmallLayout sc = sc_small_layout();
    dump("sc_small", {{"R", sc.R}, {"nu", sc.nu}, {"nis", sc.nis}, {"S", sc.S}, {"flag", sc.flag}, {"bytes", sc.bytes}});
    const BlkInLayout b = blk_in_layout();
    dump("blk_in", {{"Fr", b.Fr}, {"Qr", b.Qr}, {"dx", b.dx}, {"bytes", b.bytes}});
    const IniInLayout in = ini_in_layout();
    dump("ini_in", {{"G", in.G}, {"W", in.W}, {"xb", in.xb}, {"cols", in.cols}, {"bytes", in.bytes}});
    const RdBufLayout rd = rd_buf_layout();
    dump("rd_buf", {{"out", rd.out}, {"rows", rd.rows}, {"cols", rd.cols}, {"bytes", rd.bytes}});
    const int cases[5][5] = {{1, 1, 1, 1, 0}, {1, 2, 5, 1, 1}, {3, 2, 5, 0, 1}, {70, 3, 7, 0, 0}, {5000, 2, 5, 1, 0}};
    for (const auto& q : cases) {
        const SpsLayout l = sps_layout(q[0], q[1], q[2], q[3] != 0, q[4] != 0);
        std::string name = "sps@";
        for (int i = 0; i < 5; i++) name += (i ? "," : "") + std::to_string(q[i]);
        dump(name, {{"Hc", l.Hc}, {"R", l.R}, {"nu", l.nu}, {"nis", l.nis}, {"S", l.S}, {"cols", l.cols}, {"flag", l.flag}, {"bytes", l.bytes}});
    }
    return 0;
}
