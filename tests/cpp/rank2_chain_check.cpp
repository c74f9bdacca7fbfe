// rank2_chain_check.cpp -- host sweep of the chained pass's plan (ekf_rank2_plan.hpp: rank2_chain_plan / rank2_chain_item, what
// k_rank2_chain decodes a queue item with).  For every (B, N, m): every tile of every filter lies in exactly one item, no item
// spans two filters, the item count is the queue's `total`; and the conditions under which a step chains.  Stand-alone: no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ekf_rank2_plan.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            std::printf("FAIL %s: ", #cond);                  \
            std::printf(__VA_ARGS__);                         \
            std::printf("\n");                                \
            failures++;                                       \
        }                                                     \
    } while (0)

static ekf::Rank2Tuning tuning() { return ekf::Rank2Tuning{0, -1, 0, 1, 1, 1}; }

static void sweep_items(int B, int N, int m) {
    const int ld = ekf::pick_ld(N);
    const ekf::Rank2Plan single = ekf::rank2_plan(B, N, ld, tuning(), true, true, 256);
    const ekf::ChainPlan c = ekf::rank2_chain_plan(B, N, ld, single, true, true, true, 2, m, 0);
    const int tiles = c.chunks * c.row_blocks;
    CHECK(c.rows == ekf::kChainRows && c.row_blocks == (N + c.rows - 1) / c.rows, "B=%d N=%d", B, N);
    CHECK(c.chunks * 256 >= (N + 1) / 2 && (c.chunks - 1) * 256 < (N + 1) / 2, "B=%d N=%d chunks=%d", B, N, c.chunks);
    CHECK(c.chunks * 512 <= ld + 511, "B=%d N=%d: a column chunk beyond the row", B, N);
    CHECK(c.tiles_per_batch >= 1 && c.tiles_per_batch <= tiles, "B=%d N=%d m=%d", B, N, m);
    CHECK((long long)c.total == (long long)B * c.items_per_filter, "B=%d N=%d m=%d total=%u", B, N, m, c.total);
    CHECK(c.items_per_filter == (unsigned)((tiles + c.tiles_per_batch - 1) / c.tiles_per_batch), "B=%d N=%d m=%d", B, N, m);
    std::vector<unsigned char> seen((size_t)B * tiles, 0);
    for (unsigned s = 0; s < c.total; s++) {
        int b, first, count;
        ekf::rank2_chain_item(c, s, &b, &first, &count);
        if (!(b >= 0 && b < B && first >= 0 && count >= 1 && count <= c.tiles_per_batch && first + count <= tiles)) {
            CHECK(false, "B=%d N=%d m=%d item %u: filter %d tiles [%d, %d)", B, N, m, s, b, first, first + count);
            return;
        }
        for (int t = first; t < first + count; t++) seen[(size_t)b * tiles + t]++;
    }
    size_t bad = 0;
    for (unsigned char v : seen) bad += v != 1;
    CHECK(bad == 0, "B=%d N=%d m=%d: %zu tiles not visited exactly once", B, N, m, bad);
}

// The shapes of tests/rank2_chain_cases.py (tests/test_rank2_chain_host.py holds the printed table against that module): on
// 256 compute units, with the row's packing setting, a correction takes the tile queue, a step of two slots chains, and ld,
// column chunks, 16-row tiles and the rows of the last tile are what the case is there for.
struct Case {
    const char* name;
    int n, B, ld, chunks, row_blocks, last_rows, packing;
};

static void check_cases() {
    const Case table[] = {{"one-chunk", 250, 256, 512, 1, 32, 7, 1},  {"narrow-ld", 478, 72, 960, 2, 60, 15, 1},
                          {"one-row", 503, 64, 1024, 2, 64, 1, 1},    {"three-chunk", 700, 32, 1408, 3, 88, 11, 0},
                          {"four-chunk", 1000, 24, 2048, 4, 126, 3, 1}, {"long-call", 500, 80, 1024, 2, 63, 11, 1}};
    for (const Case& k : table) {
        const int N = 3 + 2 * k.n, ld = ekf::pick_ld(N);
        ekf::Rank2Tuning t = tuning();
        t.row_packing = k.packing;
        const ekf::Rank2Plan single = ekf::rank2_plan(k.B, N, ld, t, true, true, 256);
        const ekf::ChainPlan c = ekf::rank2_chain_plan(k.B, N, ld, single, true, true, true, 2, 0, 0);
        const int last_rows = N - (c.row_blocks - 1) * c.rows;
        CHECK(single.kind == ekf::RANK2_QUEUE, "%s: kind %d P %d", k.name, single.kind, single.P);
        CHECK(c.chains == 1, "%s does not chain", k.name);
        CHECK(ld == k.ld && c.chunks == k.chunks && c.row_blocks == k.row_blocks && last_rows == k.last_rows,
              "%s: ld %d chunks %d row blocks %d last rows %d", k.name, ld, c.chunks, c.row_blocks, last_rows);
        if (!k.packing) {   // with packing on the pool would be packed, not queued
            const ekf::Rank2Plan packed = ekf::rank2_plan(k.B, N, ld, tuning(), true, true, 256);
            CHECK(packed.kind == ekf::RANK2_PACKED, "%s: packing on gives kind %d", k.name, packed.kind);
        }
        std::printf("case %s n=%d B=%d N=%d ld=%d chunks=%d row_blocks=%d last_rows=%d packing=%d\n", k.name, k.n, k.B, N, ld,
                    c.chunks, c.row_blocks, last_rows, k.packing);
    }
    std::printf("ok cases %d\n", failures);
}

int main(int argc, char** argv) {
    const int head_n = argc > 1 ? std::atoi(argv[1]) : 1000, head_B = argc > 2 ? std::atoi(argv[2]) : 4096;
    const int shapes[][2] = {{head_B, 3 + 2 * head_n}, {24, 2003}, {80, 1003}, {70, 1005}, {1, 2003}, {3, 17}, {2, 16}, {5, 513},
                             {7, 1025}, {2, 10003}};
    for (const auto& sh : shapes)
        for (int m : {0, 1, 2, 4, 5, 8, 63, 1 << 20}) sweep_items(sh[0], sh[1], m);
    std::printf("ok items %d\n", failures);

    // when a step chains: the form on, an eager full-width pool whose single correction takes the tile queue, >= 2 slots
    const int N = 3 + 2 * head_n, ld = ekf::pick_ld(N);
    const ekf::Rank2Plan q = ekf::rank2_plan(head_B, N, ld, tuning(), true, true, 256);
    CHECK(q.kind == ekf::RANK2_QUEUE, "the headline pool is not on the tile queue");
    CHECK(ekf::rank2_chain_plan(head_B, N, ld, q, true, true, true, 2, 0, 0).chains == 1, "headline");
    CHECK(ekf::rank2_chain_plan(head_B, N, ld, q, true, true, true, 1, 0, 0).chains == 0, "one slot");
    CHECK(ekf::rank2_chain_plan(head_B, N, ld, q, false, true, true, 2, 0, 0).chains == 0, "form off");
    CHECK(ekf::rank2_chain_plan(head_B, N, ld, q, true, false, true, 2, 0, 0).chains == 0, "not eager");
    CHECK(ekf::rank2_chain_plan(head_B, N, ld, q, true, true, false, 2, 0, 0).chains == 0, "not full width");
    const ekf::Rank2Plan g = ekf::rank2_plan(2, 123, ekf::pick_ld(123), tuning(), true, true, 256);
    CHECK(g.kind != ekf::RANK2_QUEUE && ekf::rank2_chain_plan(2, 123, ekf::pick_ld(123), g, true, true, true, 2, 0, 0).chains == 0,
          "small pool");
    // policy: automatic = the last sweep's stores non-temporal where the single pass is, explicit = the bits as given
    const ekf::ChainPlan a = ekf::rank2_chain_plan(head_B, N, ld, q, true, true, true, 2, 0, 0);
    CHECK(a.policy == (q.nontemporal ? 8 : 0) && a.tiles_per_batch == 1, "automatic policy %d m %d", a.policy, a.tiles_per_batch);
    CHECK(ekf::rank2_chain_plan(head_B, N, ld, q, true, true, true, 2, 4, ekf::kChainPolicyExplicit | 5).policy == 5, "explicit");
    CHECK(ekf::rank2_chain_plan(head_B, N, ld, q, true, true, true, 2, 4, ekf::kChainPolicyExplicit).policy == 0, "explicit 0");
    std::printf("ok conditions %d\n", failures);
    check_cases();
    return failures ? 1 : 0;
}
