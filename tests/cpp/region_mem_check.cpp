// region_mem_check.cpp -- the device memory of a local region (ekf_dense64_region_mem.hpp, what ekf_dense64_region_begin
// calls) on a CPU, over a fake memory policy that hands out distinct addresses and fails the k-th allocation: the
// accumulators and the scratch come as one group or not at all.  Prints one "ok <scenario>" line per scenario; a broken
// property prints FAILED and exits non-zero (tests/test_dense64_region_host.py).
#include "ekf_dense64_region_mem.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(cond)                                                                      \
    do {                                                                                 \
        if (!(cond)) {                                                                   \
            std::printf("FAILED %s:%d [%s]: %s\n", __FILE__, __LINE__, g_scenario, #cond); \
            std::exit(1);                                                                \
        }                                                                                \
    } while (0)

static const char* g_scenario = "";

struct Fake {
    using Stream = int;
    static constexpr int kOutOfMemory = 2, kOther = 7;
    static inline uintptr_t next = 0x1000;
    static inline int allocs = 0, fail_alloc = 0, fail_code = 0, frees = 0, clears = 0;
    static inline std::vector<void*> live;
    static void arm(int k, int code) { allocs = frees = clears = 0; fail_alloc = k; fail_code = code; }
    static int alloc(void** p, size_t) {
        if (++allocs == fail_alloc) return fail_code;
        *p = reinterpret_cast<void*>(next);
        next += 0x1000;
        live.push_back(*p);
        return 0;
    }
    static int free(void* p) {
        frees++;
        for (size_t i = 0; i < live.size(); i++)
            if (live[i] == p) { live.erase(live.begin() + i); return 0; }
        std::printf("FAILED: %p freed twice or never allocated\n", p);
        std::exit(1);
    }
    static int fill(void*, int, size_t, Stream) { return 0; }
    static int sync(Stream) { return 0; }
    static void clear_error() { clears++; }
    static const char* error_string(int e) { return e == kOutOfMemory ? "out of memory" : "some other error"; }
};
using Ledger = ekfrt::DeviceLedger<Fake>;

int main() {
    const ekf::Dense64RegionPlan small = ekf::dense64_region_plan(65, 200, 256), big = ekf::dense64_region_plan(191, 403, 512);
    for (int code : {Fake::kOutOfMemory, Fake::kOther})
        for (int k : {1, 2}) {   // the first member fails, the second member fails
            // ---- from nothing
            g_scenario = "fresh";
            Ledger mem;
            ekfrt::RegionMem rm;
            Fake::arm(k, code);
            ekf_status st = rm.reserve(mem, small, "fn");
            CHECK(st == (code == Fake::kOutOfMemory ? EKF_ERR_NOMEM : EKF_ERR_HIP) && Fake::clears == 1);
            CHECK(!rm.acc && !rm.scratch && rm.held == 0 && mem.table.empty() && Fake::live.empty());
            std::printf("ok fresh code %d member %d\n", code, k);
            // ---- with the buffers of a smaller region held: they stay, to the byte
            g_scenario = "regrow";
            Fake::arm(0, 0);
            CHECK(rm.reserve(mem, small, "fn") == EKF_OK && rm.acc && rm.scratch && rm.held == small.group_bytes);
            CHECK(mem.bytes() == small.group_bytes && mem.bytes_of(rm.acc) == small.acc_bytes);
            void *a = rm.acc, *s = rm.scratch;
            Fake::arm(0, 0);
            CHECK(rm.reserve(mem, small, "fn") == EKF_OK && Fake::allocs == 0 && rm.acc == a && rm.scratch == s);   // enough: nothing
            Fake::arm(k, code);
            st = rm.reserve(mem, big, "fn");
            CHECK(st == (code == Fake::kOutOfMemory ? EKF_ERR_NOMEM : EKF_ERR_HIP) && Fake::clears == 1);
            CHECK(rm.acc == a && rm.scratch == s && rm.held == small.group_bytes);
            CHECK(mem.table.size() == 2 && mem.bytes() == small.group_bytes && Fake::live.size() == 2);
            CHECK(Fake::frees == k - 1);   // only what this call had allocated itself
            std::printf("ok regrow refused code %d member %d\n", code, k);
            Fake::arm(0, 0);
            CHECK(rm.reserve(mem, big, "fn") == EKF_OK && rm.acc != a && rm.scratch != s && rm.held == big.group_bytes);
            CHECK(mem.table.size() == 2 && mem.bytes() == big.group_bytes && Fake::frees == 2 && Fake::live.size() == 2);
            Fake::arm(0, 0);
            CHECK(rm.reserve(mem, small, "fn") == EKF_OK && Fake::allocs == 0 && rm.held == big.group_bytes);    // kept for a smaller one
            std::printf("ok regrow code %d member %d\n", code, k);
            mem.free_all();
            Fake::live.clear();
        }
    return 0;
}
