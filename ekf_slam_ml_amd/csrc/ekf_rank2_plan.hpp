// ekf_rank2_plan.hpp -- which kernel, in which shape, an eager rank-2 correction of a pool view launches.  Host only, no HIP:
// launch_rank2 (ekf_kernels.hip) launches from the plan, the report hooks (ekf_batch_rank2_variant / _resident / _packing)
// read the same plan, and tests/cpp/rank2_plan_check.cpp sweeps it on the CPU.
#pragma once
#include <cstddef>

namespace ekf {

// Leading dimension of Sigma, the factor vectors and the state: N rounded up to 16 doubles (rows on 128-byte lines), and
// to 256 doubles -- rows on 2-KB boundaries -- where that costs at most 1/32 of a row (n = 1000: 2003 -> 2048, n = 5000:
// 10003 -> 10240).  The strip-form flush reads a row as 2-KB pieces, one per workgroup: on a 2-KB boundary a piece is one
// DRAM page visit instead of two halves (48.3 -> 47.0 ms at 64 pending vectors, 46.8 -> 43.9 at 2; k_rank2 40.09 -> 39.90:
// profiles/r04/ld_alignment_ab.txt).
inline int pick_ld(int N) {
    const int wide = (N + 255) / 256 * 256;
    return (wide - N) * 32 <= N ? wide : (N + 15) / 16 * 16;
}

struct Rank2Tuning {
    int rows_per_block;  // <= 0: automatic
    int nontemporal;     // < 0: automatic
    int group_rows;      // rows per load/store group U in {2,4,8}; other values: automatic
    int row_packing;     // 1: narrow full-width views may take the row-packed kernel (EKF_FORM_ROW_PACKING)
    int strip_flush;     // delayed mode: 0 never, 1 automatic, 2 always the strip-form flush (EKF_FORM_STRIP_FLUSH*)
    int tile_queue;      // 1: big pools stream the rank-2 update as resident workgroups on one tile queue (EKF_FORM_TILE_QUEUE)
};

enum Rank2Kind { RANK2_GRID = 0, RANK2_QUEUE = 1, RANK2_PACKED = 2 };   // k_rank2 / k_rank2_queue / k_rank2_packed

// why rank2_packing chose P = 1 (the order of its tests), or that it packs
enum Rank2NoPack {
    RANK2_PACKS = 0,
    RANK2_NOPACK_FORM_OFF,      // EKF_FORM_ROW_PACKING off
    RANK2_NOPACK_SHORT_ROW,     // ld / 2 < 64: a wavefront would straddle more than two sub-rows
    RANK2_NOPACK_PREFIX,        // ld != pick_ld(N): a prefix view, columns beyond it must stay untouched
    RANK2_NOPACK_FULL_STRIPS,   // the rows fill their 256-lane strips to >= 93 % already
    RANK2_NOPACK_WORK_FLOOR,    // B * N * ld/2 < 256 * 256 * 64: too little work for fat workgroups
    RANK2_NOPACK_NO_P           // no P <= 32 fills the strips to >= 97 %
};

constexpr double kRank2PackSkip = 0.93, kRank2PackFill = 0.97;
constexpr int kRank2PackMaxP = 32;
constexpr long long kRank2PackWorkFloor = 256LL * 256 * 64;

// share of the 256-lane strips' lanes that carry a column when P rows of ld2n double2 columns are one virtual row
inline double rank2_pack_util(int P, int ld2n) {
    const long long w = (long long)P * ld2n;
    return (double)w / (double)((w + 255) / 256 * 256);
}

// P > 1: the row-packed kernel serves this (full-width) view -- the smallest P <= 32 whose virtual rows fill the
// 256-lane strips to >= 97 %; 1: the plain kernel (rows already fill their strips, rows shorter than a wavefront, or a
// small pool that needs more workgroups than packing leaves)
inline int rank2_packing(int B, int N, int ld, const Rank2Tuning& t, Rank2NoPack* why = nullptr) {
    const int ld2n = ld / 2;
    Rank2NoPack w = RANK2_PACKS;
    int P = 1;
    if (!t.row_packing) w = RANK2_NOPACK_FORM_OFF;
    else if (ld2n < 64) w = RANK2_NOPACK_SHORT_ROW;
    else if (pick_ld(N) != ld) w = RANK2_NOPACK_PREFIX;
    else if (rank2_pack_util(1, ld2n) >= kRank2PackSkip) w = RANK2_NOPACK_FULL_STRIPS;
    else if ((long long)B * N * ld2n < kRank2PackWorkFloor) w = RANK2_NOPACK_WORK_FLOOR;
    else {
        w = RANK2_NOPACK_NO_P;
        for (int p = 2; p <= kRank2PackMaxP; p++)
            if (rank2_pack_util(p, ld2n) >= kRank2PackFill) { P = p; w = RANK2_PACKS; break; }
    }
    if (why) *why = w;
    return P;
}

struct Rank2Plan {
    int kind;           // Rank2Kind
    int group_rows;     // U of the instantiation
    int nontemporal;    // NT of the instantiation
    int threads;        // workgroup size (k_rank2 / k_rank2_queue: the TPB of the instantiation; packed: 256)
    int rows;           // rows (packed: virtual rows) per workgroup / tile
    int P;              // rows per virtual row; 1 unless kind == RANK2_PACKED
    unsigned grid[3];   // the launch grid; RANK2_QUEUE: the TILE grid (chunks, row blocks, filters) -- `cus` workgroups take it
};

// B, N, ld: the view (N may be a discovered prefix of ld); full_width: the caller guarantees valid K / G over the whole row;
// has_queue: the pool owns a queue word; cus: compute units of the device (0: unknown, no tile queue)
inline Rank2Plan rank2_plan(int B, int N, int ld, const Rank2Tuning& t, bool full_width, bool has_queue, int cus) {
    Rank2Plan p{};
    // Non-temporal only when the pool cannot stay resident in the 256 MiB Infinity Cache between
    // two corrections; a single filter's covariance (32 MB at n = 1000) should stay cached.
    // (the bytes this launch touches: N may be a discovered prefix of a much larger pool)
    const size_t pool_bytes = (size_t)B * N * ((size_t)N * sizeof(double));
    p.nontemporal = (t.nontemporal >= 0 ? t.nontemporal != 0 : pool_bytes > ((size_t)192 << 20)) ? 1 : 0;
    p.P = full_width ? rank2_packing(B, N, ld, t) : 1;
    if (p.P > 1) {
        const int ld2n = ld / 2;
        // measured (tools/rank2_width_sweep.py, profiles/r02/rank2_width_sweep.txt): ONE 8-row group per workgroup
        // (n = 200, B = 16384: 6.26 TB/s = 0.78 of peak; 16 rows 0.73, 32 rows 0.64; the plain kernel 0.67)
        p.kind = RANK2_PACKED;
        p.group_rows = t.group_rows == 16 ? 16 : 8;
        p.threads = 256;
        p.rows = t.rows_per_block > 0 ? t.rows_per_block : 8;
        p.grid[0] = (unsigned)((p.P * ld2n + 255) / 256);
        p.grid[1] = (unsigned)(((N + p.P - 1) / p.P + p.rows - 1) / p.rows);
        p.grid[2] = (unsigned)B;
        return p;
    }
    int u = t.group_rows;
    int rows = t.rows_per_block;
    if (rows <= 0) {
        // Measured on MI355X (profiles/): a big pool streams fastest with 32 rows per workgroup taken as
        // two 16-row groups (32 x 16 B in flight per lane, 2 waves/SIMD): 6.17 TB/s algorithmic.  A small
        // pool needs enough workgroups to cover 256 CUs a few times over.
        const long long strips = (long long)B * (((N + 1) / 2 + 255) / 256);
        const long long total = strips * N;
        rows = total >= 256LL * 8 * 32 ? 32 : (total >= 256LL * 4 * 8 ? 8 : 4);
    }
    if (rows > 1024) rows = 1024;
    if (u != 2 && u != 4 && u != 8 && u != 16) u = rows >= 32 ? 16 : (rows >= 8 ? 8 : (rows >= 4 ? 4 : 2));
    const int ld2a = (N + 1) / 2;   // double2 columns of an active row
    const int tpb = ld2a <= 64 ? 64 : (ld2a <= 128 ? 128 : (ld2a <= 192 ? 192 : 256));
    p.group_rows = u;
    p.threads = tpb;
    p.rows = rows;
    p.grid[0] = (unsigned)((ld2a + tpb - 1) / tpb);
    p.grid[1] = (unsigned)((N + rows - 1) / rows);
    p.grid[2] = (unsigned)B;
    // resident workgroups on one tile queue (k_rank2_queue): the 256-lane, 16-row-group instantiation on pools with at
    // least 16 tiles per CU
    const long long total = (long long)p.grid[0] * p.grid[1] * p.grid[2];
    const bool resident = t.tile_queue && has_queue && u == 16 && tpb == 256 && cus > 0 && total >= 16LL * cus &&
                          total < 0x7fffffffLL;
    p.kind = resident ? RANK2_QUEUE : RANK2_GRID;
    return p;
}

// The CHAINED pass (k_rank2_chain, EKF_FORM_STEP_CHAIN): one launch applies all corrections of a step, batch of tiles by
// batch of tiles -- a resident workgroup sweeps its batch once per correction and re-loads what it stored itself while the
// lines are still on the chip.  Policy bits (non-temporal where set, plain otherwise): 1 = the first sweep's loads, 2 = the
// stores of every sweep but the last, 4 = the re-loads, 8 = the last sweep's stores.
constexpr int kChainRows = 16;          // rows of a tile: 256 CUs x 64 KB = half of the L2s (tools/micro/strip_walk.hip chain)
constexpr int kChainPolicyExplicit = 16;   // set in a policy override: the low four bits are taken as they are (0 = automatic)

struct ChainPlan {
    int chains;                 // 1: the step takes the chained pass
    int rows;                   // rows of a tile (512 columns wide)
    int tiles_per_batch;        // m: consecutive tiles of one filter per queue item (column chunks fastest)
    int policy;                 // the four policy bits
    int chunks, row_blocks;     // tiles of one filter: chunks x row_blocks
    unsigned items_per_filter;  // ceil(chunks * row_blocks / m): a filter's last batch may be short; no item spans two filters
    unsigned total;             // queue items of the launch: B * items_per_filter
};

// eager: not delayed, not call-fused, not active-set; `single` is the plan of ONE correction over the same full-width view;
// active_slots: slots of the step with a correction in at least one filter; m_override / policy_override: 0 = automatic
inline ChainPlan rank2_chain_plan(int B, int N, int ld, const Rank2Plan& single, bool form_on, bool eager, bool full_width,
                                  int active_slots, int m_override, int policy_override) {
    ChainPlan c{};
    c.rows = kChainRows;
    c.tiles_per_batch = m_override > 0 ? m_override : 1;
    c.policy = (policy_override & kChainPolicyExplicit) ? (policy_override & 15) : (single.nontemporal ? 8 : 0);
    c.chunks = ((N + 1) / 2 + 255) / 256;
    c.row_blocks = (N + c.rows - 1) / c.rows;
    const long long tiles = (long long)c.chunks * c.row_blocks;
    if (c.tiles_per_batch > tiles) c.tiles_per_batch = (int)tiles;
    const long long ipf = (tiles + c.tiles_per_batch - 1) / c.tiles_per_batch;
    const long long total = ipf * B;
    c.items_per_filter = (unsigned)ipf;
    c.total = (unsigned)total;
    c.chains = form_on && eager && full_width && single.kind == RANK2_QUEUE && active_slots >= 2 && ld % 2 == 0 &&
               total < 0x7fffffffLL;
    return c;
}

// tile range [first, first + count) of queue item s, and its filter (what k_rank2_chain decodes)
inline void rank2_chain_item(const ChainPlan& c, unsigned s, int* filter, int* first, int* count) {
    const int tiles = c.chunks * c.row_blocks;
    *filter = (int)(s / c.items_per_filter);
    *first = (int)(s % c.items_per_filter) * c.tiles_per_batch;
    *count = *first + c.tiles_per_batch < tiles ? c.tiles_per_batch : tiles - *first;
}

}  // namespace ekf
