// device_mem_check.cpp -- ekf_device_mem.hpp on a CPU: DeviceLedger, ScopedLedger and DeviceBuf over a fake memory policy
// that hands out distinct addresses, records every allocate / free / fill / synchronise / clear-error call and fails the
// k-th allocation or the k-th fill.  Prints one "ok <scenario>" line per scenario; any broken property aborts with a message
// and a non-zero exit (tests/test_device_mem_host.py).
#include "ekf_device_mem.hpp"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d [%s]: %s\n", __FILE__, __LINE__, g_scenario.c_str(), #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

static std::string g_scenario;

struct Fake {
    using Stream = int;
    static constexpr int kOutOfMemory = 2, kOther = 7;
    enum Kind { kAlloc, kFree, kFill, kSync, kClear };
    struct Ev { Kind kind; void* p; size_t bytes; int byte; bool failed; };
    static inline std::vector<Ev> log;
    static inline uintptr_t next = 0x1000;
    static inline int allocs = 0, fills = 0, fail_alloc = 0, fail_fill = 0, fail_code = 0;   // k-th call since arm(); 0 = never

    static void arm(int k_alloc, int k_fill, int code) { log.clear(); allocs = fills = 0; fail_alloc = k_alloc; fail_fill = k_fill; fail_code = code; }
    static int alloc(void** p, size_t bytes) {
        if (++allocs == fail_alloc) { log.push_back({kAlloc, nullptr, bytes, 0, true}); return fail_code; }
        *p = reinterpret_cast<void*>(next);
        next += 0x1000;   // never handed out twice
        log.push_back({kAlloc, *p, bytes, 0, false});
        return 0;
    }
    static int free(void* p) { log.push_back({kFree, p, 0, 0, false}); return 0; }
    static int fill(void* p, int byte, size_t bytes, Stream) {
        const bool bad = ++fills == fail_fill;
        log.push_back({kFill, p, bytes, byte, bad});
        return bad ? fail_code : 0;
    }
    static int sync(Stream) { log.push_back({kSync, nullptr, 0, 0, false}); return 0; }
    static void clear_error() { log.push_back({kClear, nullptr, 0, 0, false}); }
    static const char* error_string(int e) { return e == kOutOfMemory ? "out of memory" : "some other error"; }

    static int count(Kind k, const void* p = nullptr) {
        return (int)std::count_if(log.begin(), log.end(), [&](const Ev& e) { return e.kind == k && !(k == kAlloc && e.failed) && (!p || e.p == p); });
    }
};
using Ledger = ekfrt::DeviceLedger<Fake>;
using ekfrt::Fill;

// what holds of every recorded sequence: nothing freed twice, nothing filled after it was freed
static void audit_log() {
    std::set<void*> freed;
    for (const Fake::Ev& e : Fake::log) {
        if (e.kind == Fake::kFill) CHECK(!freed.count(e.p));
        if (e.kind == Fake::kFree) CHECK(freed.insert(e.p).second);
    }
}

// after a failed call: the last thing that happened is the clearing of the API's error; status and text follow the code
static void check_refusal(ekf_status st, int code) {
    CHECK(st == (code == Fake::kOutOfMemory ? EKF_ERR_NOMEM : EKF_ERR_HIP));
    CHECK(!Fake::log.empty() && Fake::log.back().kind == Fake::kClear);
    CHECK(ekfrt::g_err == std::string("fn: ") + Fake::error_string(code) + " while reserving what");
}

// ---- replace_group of n targets, fill of target i = kinds[i % 3]; the targets are live before (so the release counts) --------
static const Fill kKinds[3] = {Fill::kZero, Fill::kNone, Fill::kOnes};
static size_t size_of(int i) { return 64 + 24 * (size_t)i; }

static void group_case(int n, int k_alloc, int k_fill, int code) {
    g_scenario = "group n=" + std::to_string(n) + " alloc#" + std::to_string(k_alloc) + " fill#" + std::to_string(k_fill) + " code " + std::to_string(code);
    Fake::arm(0, 0, 0);
    Ledger mem;
    mem.stream = 5;
    char* by = nullptr;   // a bystander: never touched
    CHECK(mem.alloc(&by, 1000, Fill::kNone, "fn", "what") == EKF_OK);
    double* t[9] = {};
    size_t old_sum = 0;
    std::vector<void*> old;
    for (int i = 0; i < n; i++) {
        CHECK(mem.alloc(&t[i], 3 + i, Fill::kNone, "fn", "what") == EKF_OK);
        old.push_back(t[i]);
        old_sum += sizeof(double) * (3 + i);
    }
    const size_t before = mem.bytes();
    CHECK(before == 1000 + old_sum);
    Fake::arm(k_alloc, k_fill, code);
    auto T = [&](int i) { return ekfrt::target_bytes(&t[i], size_of(i), kKinds[i % 3]); };
    const ekf_status st = n == 1   ? mem.replace_group({T(0)}, "fn", "what")
                          : n == 3 ? mem.replace_group({T(0), T(1), T(2)}, "fn", "what")
                                   : mem.replace_group({T(0), T(1), T(2), T(3), T(4), T(5), T(6), T(7), T(8)}, "fn", "what");
    audit_log();
    for (void* o : old) CHECK(Fake::count(Fake::kFree, o) == 1);   // released first, once
    CHECK(Fake::count(Fake::kFree, by) == 0);
    int n_fill = 0;
    size_t new_sum = 0;
    for (int i = 0; i < n; i++) { n_fill += kKinds[i % 3] != Fill::kNone; new_sum += size_of(i); }
    const bool failing = (k_alloc >= 1 && k_alloc <= n) || (k_fill >= 1 && k_fill <= n_fill);
    if (failing) {
        check_refusal(st, code);
        for (int i = 0; i < n; i++) CHECK(t[i] == nullptr);
        CHECK(mem.bytes() == before - old_sum);
        for (const Fake::Ev& e : Fake::log)   // every fresh allocation went back, once (audit_log: not twice)
            if (e.kind == Fake::kAlloc && !e.failed) CHECK(Fake::count(Fake::kFree, e.p) == 1);
        // the fresh buffers are freed behind a synchronisation: fills may be in flight
        bool synced = false;
        for (const Fake::Ev& e : Fake::log) {
            if (e.kind == Fake::kSync) synced = true;
            if (e.kind == Fake::kFree && std::find(old.begin(), old.end(), e.p) == old.end()) CHECK(synced);
        }
    } else {
        CHECK(st == EKF_OK);
        CHECK(Fake::count(Fake::kClear) == 0 && Fake::count(Fake::kFree) == n);
        std::set<void*> seen(old.begin(), old.end());
        seen.insert(by);
        for (int i = 0; i < n; i++) CHECK(t[i] != nullptr && seen.insert(t[i]).second);   // non-null, distinct, new
        CHECK(mem.bytes() == before - old_sum + new_sum);
        // each fill directly follows its own allocation, with its byte and its size
        size_t at = (size_t)n;   // (the n releases come first)
        for (int i = 0; i < n; i++) {
            CHECK(at < Fake::log.size() && Fake::log[at].kind == Fake::kAlloc && Fake::log[at].p == t[i] && Fake::log[at].bytes == size_of(i));
            at++;
            if (kKinds[i % 3] == Fill::kNone) continue;
            const Fake::Ev& f = Fake::log[at++];
            CHECK(f.kind == Fake::kFill && f.p == t[i] && f.bytes == size_of(i) && f.byte == (int)kKinds[i % 3]);
        }
        CHECK(at == Fake::log.size());
    }
    mem.free_all();
}

static void group_scenarios() {
    for (int n : {1, 3, 9}) {
        int n_fill = 0;
        for (int i = 0; i < n; i++) n_fill += kKinds[i % 3] != Fill::kNone;
        group_case(n, 0, 0, 0);
        for (int code : {Fake::kOutOfMemory, Fake::kOther}) {
            for (int k = 1; k <= n; k++) group_case(n, k, 0, code);
            for (int k = 1; k <= n_fill; k++) group_case(n, 0, k, code);
        }
        std::printf("ok replace_group %d\n", n);
    }
}

// ---- grow ---------------------------------------------------------------------------------------------------------------
static void grow_case(int k_alloc, int k_fill, int code) {
    g_scenario = "grow alloc#" + std::to_string(k_alloc) + " fill#" + std::to_string(k_fill) + " code " + std::to_string(code);
    Fake::arm(0, 0, 0);
    Ledger mem;
    int* p = nullptr;
    CHECK(mem.alloc(&p, 25, Fill::kNone, "fn", "what") == EKF_OK);
    int* const old = p;
    Fake::arm(k_alloc, k_fill, code);
    CHECK(mem.grow(&p, 25, Fill::kZero, "fn", "what") == EKF_OK && mem.grow(&p, 7, Fill::kZero, "fn", "what") == EKF_OK);
    CHECK(Fake::log.empty() && p == old);   // large enough already: no call at all
    Fake::arm(k_alloc, k_fill, code);
    const ekf_status st = mem.grow(&p, 50, Fill::kZero, "fn", "what");
    audit_log();
    if (k_alloc == 1 || k_fill == 1) {
        check_refusal(st, code);
        CHECK(p == old && mem.bytes_of(p) == 100 && mem.bytes() == 100 && Fake::count(Fake::kFree, old) == 0);
        if (k_fill == 1) {   // allocate, fill (fails), synchronise, free the fresh buffer, clear
            CHECK(Fake::log.size() == 5 && Fake::log[2].kind == Fake::kSync && Fake::log[3].kind == Fake::kFree && Fake::log[3].p == Fake::log[0].p);
        } else {
            CHECK(Fake::count(Fake::kFree) == 0);
        }
    } else {
        CHECK(st == EKF_OK && p != old && p != nullptr && mem.bytes_of(p) == 200 && mem.bytes() == 200);
        CHECK(Fake::count(Fake::kFree, old) == 1 && Fake::count(Fake::kFree) == 1);
        CHECK(Fake::log.size() == 3 && Fake::log[0].kind == Fake::kAlloc && Fake::log[1].kind == Fake::kFill && Fake::log[1].p == p && Fake::log[2].kind == Fake::kFree);
    }
    // DeviceBuf: the same order behind reserve; its members change only on success
    ekfrt::DeviceBuf buf;
    Fake::arm(0, 0, 0);
    CHECK(buf.reserve(mem, 40, true, "fn", "what") == EKF_OK && buf.p && buf.bytes == 40);
    void* const first = buf.p;
    Fake::arm(k_alloc, k_fill, code);
    CHECK(buf.reserve(mem, 40, true, "fn", "what") == EKF_OK && Fake::log.empty());
    const ekf_status sb = buf.reserve(mem, 80, true, "fn", "what");
    audit_log();
    if (k_alloc == 1 || k_fill == 1) {
        check_refusal(sb, code);
        CHECK(buf.p == first && buf.bytes == 40 && Fake::count(Fake::kFree, first) == 0);
    } else {
        CHECK(sb == EKF_OK && buf.p != first && buf.bytes == 80 && Fake::count(Fake::kFree, first) == 1);
    }
    mem.free_all();
}

// ---- the scoped form ------------------------------------------------------------------------------------------------------
static ekf_status scoped_body(bool leave_early, void** a, void** b) {
    ekfrt::ScopedLedger<Fake> tmp(3);
    char *x = nullptr, *y = nullptr;
    if (tmp.alloc(&x, 10, Fill::kZero, "fn", "what") != EKF_OK) return EKF_ERR_HIP;
    *a = x;
    if (leave_early) return EKF_ERR_INVALID;
    if (tmp.alloc(&y, 20, Fill::kNone, "fn", "what") != EKF_OK) return EKF_ERR_HIP;
    *b = y;
    return EKF_OK;
}

static void scoped_scenarios() {
    g_scenario = "scoped";
    for (bool early : {false, true}) {
        void *a = nullptr, *b = nullptr;
        Fake::arm(0, 0, 0);
        CHECK(scoped_body(early, &a, &b) == (early ? EKF_ERR_INVALID : EKF_OK));
        audit_log();
        CHECK(a && Fake::count(Fake::kFree, a) == 1 && Fake::count(Fake::kFree) == (early ? 1 : 2));
        if (!early) CHECK(b && Fake::count(Fake::kFree, b) == 1);
    }
    void *a = nullptr, *b = nullptr;   // the second allocation fails: the first still goes with the scope
    Fake::arm(2, 0, Fake::kOutOfMemory);
    CHECK(scoped_body(false, &a, &b) == EKF_ERR_HIP && a && !b && Fake::count(Fake::kFree, a) == 1);
    std::printf("ok scoped\n");
}

// ---- free, swapped pointers, free_all twice ---------------------------------------------------------------------------------
static void other_scenarios() {
    g_scenario = "other";
    Fake::arm(0, 0, 0);
    Ledger mem;
    double *a = nullptr, *b = nullptr, *c = nullptr;
    CHECK(mem.alloc(&a, 1, Fill::kNone, "fn", "what") == EKF_OK && mem.alloc(&b, 2, Fill::kNone, "fn", "what") == EKF_OK &&
          mem.alloc(&c, 4, Fill::kNone, "fn", "what") == EKF_OK);
    CHECK(mem.bytes() == 56 && mem.table.size() == 3);
    double* const b0 = b;
    mem.free(&b);
    CHECK(b == nullptr && Fake::count(Fake::kFree) == 1 && Fake::count(Fake::kFree, b0) == 1);
    CHECK(mem.bytes() == 40 && mem.table.size() == 2 && mem.bytes_of(a) == 8 && mem.bytes_of(c) == 32 && mem.bytes_of(b0) == 0);
    mem.free(&b);   // null: nothing
    CHECK(Fake::count(Fake::kFree) == 1);
    double* inside = c + 1;   // a pointer into a block was never entered: it is not freed
    mem.free(&inside);
    CHECK(Fake::count(Fake::kFree) == 1 && mem.table.size() == 2);
    double *a0 = a, *c0 = c;
    std::swap(a, c);   // the ping-pong of the callers: the table goes by address
    mem.free_all();
    CHECK(Fake::count(Fake::kFree, a0) == 1 && Fake::count(Fake::kFree, c0) == 1 && Fake::count(Fake::kFree) == 3 && mem.bytes() == 0);
    mem.free_all();
    CHECK(Fake::count(Fake::kFree) == 3);
    audit_log();
    std::printf("ok other\n");
}

int main() {
    group_scenarios();
    grow_case(0, 0, 0);
    for (int code : {Fake::kOutOfMemory, Fake::kOther}) {
        grow_case(1, 0, code);
        grow_case(0, 1, code);
    }
    std::printf("ok grow\n");
    scoped_scenarios();
    other_scenarios();
    return 0;
}
