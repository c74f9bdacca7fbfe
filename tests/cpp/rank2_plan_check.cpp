// rank2_plan_check.cpp -- ekf_rank2_plan.hpp on a CPU: the plan launch_rank2 launches from and the report hooks read, swept
// over N = 3 .. 2049 (odd), a few pool sizes and every tuning setting, against the rules as the header's comments state
// them, restated here in integers.  usage: rank2_plan_check <n of the benchmark's headline pool> <its B>.
// Prints one "ok <property>" line per property, then "table n B_min P ld2n" for n = 30 .. 400 (B_min: the smallest pool that
// packs; pools that never pack are left out) and "resident n=376 ..." (the smallest pools of the report-hook case); any
// broken property aborts with a message and a non-zero exit (tests/test_rank2_plan_host.py).
#include "ekf_rank2_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        if (!(cond)) {                                                                                      \
            std::printf("FAILED %s:%d [%s]: %s\n", __FILE__, __LINE__, g_where.c_str(), #cond);             \
            std::exit(1);                                                                                   \
        }                                                                                                   \
    } while (0)

static std::string g_where;
static const int kCus = 256;   // MI355X

static long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
// util(P) >= pct / 100 in integers: P * ld2n columns against the lanes of the 256-lane strips that hold them
static bool fills(int P, int ld2n, int pct) {
    const long long w = (long long)P * ld2n;
    return 100 * w >= pct * ceil_div(w, 256) * 256;
}

// the header's comment, rule by rule, in its order
static ekf::Rank2NoPack expected_reason(int B, int N, int ld, const ekf::Rank2Tuning& t, int* P_out) {
    *P_out = 1;
    const int ld2n = ld / 2;
    if (!t.row_packing) return ekf::RANK2_NOPACK_FORM_OFF;
    if (ld2n < 64) return ekf::RANK2_NOPACK_SHORT_ROW;
    if (ekf::pick_ld(N) != ld) return ekf::RANK2_NOPACK_PREFIX;
    if (fills(1, ld2n, 93)) return ekf::RANK2_NOPACK_FULL_STRIPS;
    if ((long long)B * N * ld2n < 256LL * 256 * 64) return ekf::RANK2_NOPACK_WORK_FLOOR;
    for (int P = 2; P <= 32; P++)
        if (fills(P, ld2n, 97)) { *P_out = P; return ekf::RANK2_PACKS; }
    return ekf::RANK2_NOPACK_NO_P;
}

static void describe(int B, int N, int ld, const ekf::Rank2Tuning& t, bool fw) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "B=%d N=%d ld=%d tuning=(%d,%d,%d,%d,%d) full_width=%d", B, N, ld, t.rows_per_block, t.nontemporal,
                  t.group_rows, t.row_packing, t.tile_queue, (int)fw);
    g_where = buf;
}

static bool same(const ekf::Rank2Plan& a, const ekf::Rank2Plan& b) {
    return a.kind == b.kind && a.group_rows == b.group_rows && a.nontemporal == b.nontemporal && a.threads == b.threads &&
           a.rows == b.rows && a.P == b.P && a.grid[0] == b.grid[0] && a.grid[1] == b.grid[1] && a.grid[2] == b.grid[2];
}

// one plan against everything that must hold for it; returns the reason
static ekf::Rank2NoPack check_plan(int B, int N, int ld, const ekf::Rank2Tuning& t, bool has_queue) {
    describe(B, N, ld, t, true);
    int P_want = 1;
    const ekf::Rank2NoPack want = expected_reason(B, N, ld, t, &P_want);
    ekf::Rank2NoPack why = ekf::RANK2_PACKS;
    const int P = ekf::rank2_packing(B, N, ld, t, &why);
    CHECK(why == want);
    CHECK(P == P_want);
    CHECK((P > 1) == (why == ekf::RANK2_PACKS));
    const ekf::Rank2Plan p = ekf::rank2_plan(B, N, ld, t, true, has_queue, kCus);
    CHECK(p.P == P);
    CHECK(p.grid[2] == (unsigned)B);
    CHECK(p.nontemporal == 0 || p.nontemporal == 1);
    if (t.nontemporal >= 0) CHECK(p.nontemporal == (t.nontemporal != 0));
    if (P > 1) {
        const int ld2n = ld / 2;
        CHECK(p.kind == ekf::RANK2_PACKED);
        CHECK(p.kind != ekf::RANK2_QUEUE);
        CHECK(fills(P, ld2n, 97));
        CHECK(ekf::rank2_pack_util(P, ld2n) >= 0.97);
        for (int q = 2; q < P; q++) {
            CHECK(!fills(q, ld2n, 97));
            CHECK(ekf::rank2_pack_util(q, ld2n) < 0.97);
        }
        CHECK(ld2n >= 64 && P <= 32);          // a wavefront straddles at most two sub-rows
        CHECK(p.threads == 256);
        CHECK(p.group_rows == (t.group_rows == 16 ? 16 : 8));
        CHECK(p.rows == (t.rows_per_block > 0 ? t.rows_per_block : 8));
        const long long width = (long long)P * ld2n, vrows = ceil_div(N, P);
        CHECK((long long)p.grid[0] * 256 >= width && ((long long)p.grid[0] - 1) * 256 < width);   // every slot, no idle strip
        CHECK((long long)p.grid[1] * p.rows >= vrows && ((long long)p.grid[1] - 1) * p.rows < vrows);   // ceil(N / P) virtual rows
        CHECK(vrows * P >= N && (vrows - 1) * P < N);
    } else {
        CHECK(p.kind == ekf::RANK2_GRID || p.kind == ekf::RANK2_QUEUE);
        CHECK(p.threads == 64 || p.threads == 128 || p.threads == 192 || p.threads == 256);
        CHECK(p.group_rows == 2 || p.group_rows == 4 || p.group_rows == 8 || p.group_rows == 16);
        CHECK(p.rows >= 1 && p.rows <= 1024);
        const long long cols = (N + 1) / 2;
        CHECK((long long)p.grid[0] * p.threads >= cols && ((long long)p.grid[0] - 1) * p.threads < cols);
        CHECK((long long)p.grid[1] * p.rows >= N && ((long long)p.grid[1] - 1) * p.rows < N);
        const long long tiles = (long long)p.grid[0] * p.grid[1] * p.grid[2];
        const bool queue = t.tile_queue && has_queue && p.group_rows == 16 && p.threads == 256 && tiles >= 16LL * kCus && tiles < 0x7fffffffLL;
        CHECK((p.kind == ekf::RANK2_QUEUE) == queue);
        CHECK(ekf::rank2_plan(B, N, ld, t, true, has_queue, 0).kind == ekf::RANK2_GRID);   // no CU count, no resident grid
    }
    // a launch that is not full-width never packs, and is the full-width plan wherever that one does not pack
    describe(B, N, ld, t, false);
    const ekf::Rank2Plan v = ekf::rank2_plan(B, N, ld, t, false, has_queue, kCus);
    CHECK(v.P == 1 && v.kind != ekf::RANK2_PACKED);
    if (P == 1) CHECK(same(v, p));
    ekf::Rank2Tuning off = t;
    off.row_packing = 0;
    CHECK(same(v, ekf::rank2_plan(B, N, ld, off, true, has_queue, kCus)));   // EKF_FORM_ROW_PACKING off: the same plan
    return why;
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::printf("usage: rank2_plan_check <n> <B>\n");
        return 2;
    }
    const int n_bench = std::atoi(argv[1]), B_bench = std::atoi(argv[2]);
    const ekf::Rank2Tuning dflt{0, -1, 0, 1, 1, 1};   // a pool's tuning as it is created

    // ---- the sweep ----
    long long fired[7] = {0, 0, 0, 0, 0, 0, 0}, plans = 0;
    const int Bs[] = {1, 7, 64, 540, 4096, 65535};
    const int rows_set[] = {0, 3, 8, 32, 2000}, nt_set[] = {-1, 0, 1}, group_set[] = {0, 2, 4, 8, 16};
    for (int N = 3; N <= 2049; N += 2)
        for (int B : Bs)
            for (int rows : rows_set)
                for (int nt : nt_set)
                    for (int group : group_set)
                        for (int packing = 0; packing < 2; packing++)
                            for (int queue = 0; queue < 2; queue++) {
                                const ekf::Rank2Tuning t{rows, nt, group, packing, 1, queue};
                                fired[check_plan(B, N, ekf::pick_ld(N), t, true)]++;
                                plans++;
                            }
    for (int r = 0; r < 7; r++) {
        g_where = "reason " + std::to_string(r) + " in the sweep";
        // (prefix views have a loop of their own below.  "No P <= 32 reaches 0.97" cannot fire on a pool's own ld: pick_ld
        // returns multiples of 16, so ld2n is a multiple of 8 and 32 rows are a whole number of 256-lane strips.)
        if (r == ekf::RANK2_NOPACK_PREFIX || r == ekf::RANK2_NOPACK_NO_P) CHECK(fired[r] == 0);
        else CHECK(fired[r] > 0);
    }
    std::printf("ok sweep %lld plans\n", plans);

    // ---- prefix views: N below the pool's own, on the pool's ld ----
    long long prefixes = 0, prefix_same_ld = 0;
    for (int Nfull = 131; Nfull <= 2049; Nfull += 62)
        for (int N = 3; N < Nfull; N += 2) {
            const int ld = ekf::pick_ld(Nfull);
            const ekf::Rank2NoPack why = check_plan(4096, N, ld, dflt, true);
            if (ekf::pick_ld(N) != ld) {
                CHECK(why == ekf::RANK2_NOPACK_PREFIX);
                prefixes++;
            } else {
                CHECK(why != ekf::RANK2_NOPACK_PREFIX);
                prefix_same_ld++;
            }
        }
    g_where = "prefix views";
    CHECK(prefixes > 0 && prefix_same_ld > 0);
    std::printf("ok prefix views %lld\n", prefixes);

    // ---- the work floor at its exact edge: the largest B below it and the smallest B at it ----
    long long edges = 0;
    for (int N = 3; N <= 2049; N += 2) {
        const int ld = ekf::pick_ld(N), ld2n = ld / 2;
        if (ld2n < 64 || fills(1, ld2n, 93)) continue;
        const long long B_min = ceil_div(256LL * 256 * 64, (long long)N * ld2n);
        if (B_min < 2 || B_min > 65535) continue;
        CHECK(B_min * N * ld2n >= 256LL * 256 * 64 && (B_min - 1) * N * ld2n < 256LL * 256 * 64);
        CHECK(check_plan((int)B_min - 1, N, ld, dflt, true) == ekf::RANK2_NOPACK_WORK_FLOOR);
        const ekf::Rank2NoPack at = check_plan((int)B_min, N, ld, dflt, true);
        CHECK(at == ekf::RANK2_PACKS);
        edges++;
    }
    g_where = "work floor";
    CHECK(edges > 100);
    std::printf("ok work floor edges %lld\n", edges);

    // ---- the benchmark's headline pool: the tile queue, not packed ----
    {
        const int N = 3 + 2 * n_bench, ld = ekf::pick_ld(N);
        describe(B_bench, N, ld, dflt, true);
        const ekf::Rank2Plan p = ekf::rank2_plan(B_bench, N, ld, dflt, true, true, kCus);
        CHECK(p.kind == ekf::RANK2_QUEUE && p.P == 1);
        std::printf("ok headline n=%d B=%d k_rank2_queue<%d,%s,%d> rows %d\n", n_bench, B_bench, p.group_rows, p.nontemporal ? "true" : "false",
                    p.threads, p.rows);
    }

    // ---- the table: the smallest pool of each map size that packs, and its P ----
    for (int n = 30; n <= 400; n++) {
        const int N = 3 + 2 * n, ld = ekf::pick_ld(N), ld2n = ld / 2;
        const long long B_min = ceil_div(256LL * 256 * 64, (long long)N * ld2n);
        if (B_min > 65535) continue;
        const int P = ekf::rank2_packing((int)B_min, N, ld, dflt);
        if (P > 1) std::printf("table %d %lld %d %d\n", n, B_min, P, ld2n);
    }

    // ---- the report-hook case: n = 376 packs (util(1) < 0.93) on pools big enough for the tile queue ----
    {
        const int n = 376, N = 3 + 2 * n, ld = ekf::pick_ld(N);
        ekf::Rank2Tuning off = dflt;
        off.row_packing = 0;
        int B_res = 0;
        for (int B = 1; B <= 65535 && !B_res; B++)
            if (ekf::rank2_plan(B, N, ld, off, true, true, kCus).kind == ekf::RANK2_QUEUE) B_res = B;
        describe(B_res, N, ld, dflt, true);
        CHECK(B_res > 1);
        CHECK(ekf::rank2_plan(B_res - 1, N, ld, off, true, true, kCus).kind == ekf::RANK2_GRID);
        const ekf::Rank2Plan on = ekf::rank2_plan(B_res, N, ld, dflt, true, true, kCus);
        CHECK(on.kind == ekf::RANK2_PACKED && on.P > 1);   // packing on: packed, not the queue
        std::printf("resident n=%d B_min=%d P=%d\n", n, B_res, on.P);
    }
    return 0;
}
