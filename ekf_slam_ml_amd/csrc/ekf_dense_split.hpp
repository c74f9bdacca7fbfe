// ekf_dense_split.hpp -- how one ld x ld product of the dense propagation (ekf_dense_gemm.hpp, ekf_dense.hip) is cut into
// tiles and in which order they run, for both element types.  Pure integer arithmetic, nothing from HIP (the functions are
// __host__ __device__ only under hipcc): tests/cpp/dense_split_dump.cpp walks every list on a CPU and
// tests/test_dense_split_host.py checks that each 128 x 128 block of C has exactly one owner.
#pragma once

#ifdef __HIPCC__
#define EKF_DENSE_HD __host__ __device__
#else
#define EKF_DENSE_HD
#endif

namespace ekf {
constexpr int kDenseTile = 128;   // ld must be a multiple of this; the unit of dense_gemm_split and dense_gemm_tile_map
constexpr int kDenseQuarter = 64; // edge of the tail kernel's tiles
// rows of the main kernel's tile (its columns: kDenseTile).  fp32: 256 (ekf_dense_gemm.hpp: its LDS traffic asks for the
// larger tile); fp64: 128 (sized by registers)
template <class E> inline constexpr int kDenseMainRows = 0;
template <> inline constexpr int kDenseMainRows<float> = 256;
template <> inline constexpr int kDenseMainRows<double> = 128;

// Main-tile id -> (tm, tn), tm in units of the main tile's rows, tn in units of 128 columns: the list is walked in groups of
// GROUP_M tile rows so that the A panel and the B panel of neighbouring tiles are re-used out of L2 (speed only).
EKF_DENSE_HD inline void big_tile_of(int id, int tiles_m, int tiles_n, int& tm, int& tn) {
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * tiles_n;
    const int g = id / per_group;
    const int first_m = g * GROUP_M;
    const int gm = (tiles_m - first_m) < GROUP_M ? (tiles_m - first_m) : GROUP_M;
    const int in_g = id % per_group;
    tm = first_m + in_g % gm;
    tn = in_g / gm;
}

// Consecutive workgroup ids are dealt round-robin to the 8 XCDs: remapped so that every XCD owns a contiguous chunk of the
// (grouped) main-tile list and re-uses its panels out of its own L2.  A permutation of [0, n_big).
EKF_DENSE_HD inline int xcd_remap(int id, int n_big) { return n_big % 8 == 0 ? (id % 8) * (n_big / 8) + id / 8 : id; }

// How one product is cut (make_split): the ld/BM x ld/128 list of BM x 128 main tiles (BM = kDenseMainRows) runs as whole
// rounds of resident workgroups on the main kernel (ids [0, n_big)); what is left of the list (rem_big tiles = BM/128 tiles
// of 128 x 128 each) and, when ld is no multiple of BM, the bottom strip of ld/128 tiles of 128 x 128 make the small-tile list
// of the tail kernel, which cuts each of them into four 64 x 64 quarters.  At BM = 128 there is no bottom strip.
struct DenseSplit {
    int ld, tiles_n, tiles_m, n_big, rem_big, bottom, n_small;
    int n_rows;   // rows of C that are not padding (N): the K loop stops there, and a quarter tile that lies wholly below
                  // them is not computed -- its rows of C are products of A's zero padding and stay the zeros they were
                  // allocated as
};

template <class E>
inline DenseSplit make_split(int ld, int n_rows = 0) {
    constexpr int BM = kDenseMainRows<E>;
    DenseSplit sp{};
    sp.ld = ld;
    sp.n_rows = n_rows > 0 ? n_rows : ld;
    sp.tiles_n = ld / kDenseTile;
    sp.tiles_m = ld / BM;
    sp.bottom = (ld % BM) ? 1 : 0;
    const int total_big = sp.tiles_m * sp.tiles_n;
    const int slots = 256 * 2;   // resident workgroups: __launch_bounds__ of k_gemm_big on 256 CUs
    int n_big = total_big / slots * slots;
    if (n_big == 0) n_big = total_big;   // (less than one round: all of it on the main kernel)
    sp.n_big = n_big;
    sp.rem_big = total_big - n_big;
    sp.n_small = BM / kDenseTile * sp.rem_big + sp.bottom * sp.tiles_n;
    return sp;
}

// origin of small tile q (units: elements)
template <class E>
EKF_DENSE_HD inline void small_tile_origin(const DenseSplit& sp, int q, int& row0, int& col0) {
    constexpr int BM = kDenseMainRows<E>, PER = BM / kDenseTile;   // small tiles per left-over main tile: 1 or 2
    static_assert(PER == 1 || PER == 2, "the shift below");
    if (PER == 1 || q < PER * sp.rem_big) {
        int tm, tn;
        big_tile_of(sp.n_big + (q >> (PER - 1)), sp.tiles_m, sp.tiles_n, tm, tn);
        row0 = tm * BM + (q & (PER - 1)) * kDenseTile;
        col0 = tn * kDenseTile;
    } else {
        row0 = sp.tiles_m * BM;
        col0 = (q - PER * sp.rem_big) * kDenseTile;
    }
}

// map [tiles_n][tiles_n] over the 128 x 128 blocks of C: 0 = computed by the main kernel, 1 = by the tail kernel (255 never)
template <class E>
inline void dense_tile_map(const DenseSplit& sp, unsigned char* map) {
    constexpr int PER = kDenseMainRows<E> / kDenseTile;
    const int t = sp.tiles_n;
    for (int i = 0; i < t * t; i++) map[i] = 255;
    for (int id = 0; id < sp.n_big; id++) {   // (the XCD remap permutes ids inside [0, n_big): the set of tiles is the same)
        int tm, tn;
        big_tile_of(id, sp.tiles_m, sp.tiles_n, tm, tn);
        for (int h = 0; h < PER; h++) map[(PER * tm + h) * t + tn] = 0;
    }
    for (int q = 0; q < sp.n_small; q++) {
        int r0, c0;
        small_tile_origin<E>(sp, q, r0, c0);
        map[(r0 / kDenseTile) * t + c0 / kDenseTile] = 1;
    }
}
}  // namespace ekf
