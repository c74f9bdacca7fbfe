// ekf_dense64_region.hpp -- the plan of a local region of the fp64 dense handle (ekf_dense64_region_begin ..
// ekf_dense64_region_end, include/ekfslam.h; kernels in ekf_dense64_region.hip): how the accumulators Phi, Psi, theta of the
// compressed filter and the scratch of the global update are cut and where they sit.  Pure arithmetic, nothing from HIP:
// tests/test_dense64_region_host.py compiles a plain C++17 program against it on a CPU and checks what it prints.
//   A = [0, Na) the region, B = [Na, N) the rest.  Phi, Psi: Na x Na row-major with row pitch `pitch` = Na rounded up to
//   128 doubles; theta: `pitch` doubles; W, Z: the panels of one correction, [64][pitch] each.  Nothing of these depends on
//   N or ld.  The scratch of the global update is two panels [Na][ld]: Y = -(Psi Sigma0_ab), later (Sigma0_ba Phi^T)^T, and
//   V = Phi Sigma0_ab.
#pragma once
#include <stddef.h>

namespace ekf {
constexpr int kDense64RegionMinNa = 3;        // a pose at least
constexpr int kDense64RegionTileRows = 32;    // the accumulator pass of a correction: rows ...
constexpr int kDense64RegionTileCols = 64;    // ... and columns of a workgroup's tile of the Phi / Psi pair
constexpr int kDense64RegionThreads = 256;
constexpr int kDense64RegionPanelCols = 32;   // columns of W, Z and theta a workgroup of the panel launch makes
constexpr int kDense64RegionGemmTile = 128;   // the Sigma_bb product runs on Sigma's own 128-grid ...
constexpr int kDense64RegionGemmBK = 16;      // ... with K = Na padded to the fp64 tile's BK

struct Dense64RegionPlan {
    int Na, N, ld, nb;        // nb = N - Na
    int pitch;                // row pitch of Phi, Psi, W, Z in doubles
    int upd_tiles_r, upd_tiles_c;   // the accumulator pass: tiles of 32 x 64 over Na x Na
    int panel_groups;         // workgroups of the panel launch: ceil(Na / 32)
    int map_groups;           // workgroups of a row map: ceil(Na / 256)
    int gemm_tile0;           // first tile row / column of Sigma's 128-grid that holds an index >= Na
    int gemm_tiles;           // tiles a side from there to the last one that holds an index < N
    int gemm_k;               // Na rounded up to 16
    size_t off_phi, off_psi, off_theta, off_W, off_Z, acc_bytes;   // byte offsets inside the accumulator buffer
    size_t off_Y, off_V, scratch_bytes;                            // byte offsets inside the scratch
    size_t group_bytes;       // acc_bytes + scratch_bytes: what the handle's ledger holds for the region
};

inline Dense64RegionPlan dense64_region_plan(int Na, int N, int ld) {
    Dense64RegionPlan p{};
    p.Na = Na, p.N = N, p.ld = ld, p.nb = N - Na;
    p.pitch = (Na + 127) / 128 * 128;
    p.upd_tiles_r = (Na + kDense64RegionTileRows - 1) / kDense64RegionTileRows;
    p.upd_tiles_c = (Na + kDense64RegionTileCols - 1) / kDense64RegionTileCols;
    p.panel_groups = (Na + kDense64RegionPanelCols - 1) / kDense64RegionPanelCols;
    p.map_groups = (Na + kDense64RegionThreads - 1) / kDense64RegionThreads;
    p.gemm_tile0 = Na / kDense64RegionGemmTile;
    p.gemm_tiles = (N + kDense64RegionGemmTile - 1) / kDense64RegionGemmTile - p.gemm_tile0;
    p.gemm_k = (Na + kDense64RegionGemmBK - 1) / kDense64RegionGemmBK * kDense64RegionGemmBK;
    const size_t f = sizeof(double), sq = f * (size_t)Na * p.pitch, row = f * (size_t)p.pitch;
    p.off_phi = 0, p.off_psi = sq, p.off_theta = 2 * sq, p.off_W = 2 * sq + row, p.off_Z = p.off_W + 64 * row;
    p.acc_bytes = p.off_Z + 64 * row;
    p.off_Y = 0, p.off_V = f * (size_t)Na * ld, p.scratch_bytes = 2 * p.off_V;
    p.group_bytes = p.acc_bytes + p.scratch_bytes;
    return p;
}

// an entry (i, j) of the Phi / Psi pair is read and written iff both indices are below Na: the rule of the live launches
inline bool dense64_region_masked(const Dense64RegionPlan& p, int i, int j) { return i >= p.Na || j >= p.Na; }
}  // namespace ekf
