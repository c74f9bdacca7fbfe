// ekf_device_mem.hpp -- who owns device memory (host only, no kernels, no HIP types): DeviceLedger is the table of
// {pointer, bytes} of everything a pool, a dense handle or one call allocated, and the one place where device memory is
// allocated, filled, regrown and freed.  Callers keep plain typed pointers; the table is keyed by address, so swapping two
// of them is harmless, and a pointer INTO a block is never entered.  A buffer or a group of buffers is either complete
// and initialised or absent: nothing a failed call leaves behind is partly built.  The API behind it is the policy Mem
// (ekf_runtime.hpp: HipMem; tests/cpp/device_mem_check.cpp: a recording fake):
//   Stream; kOutOfMemory; int alloc(void**, size_t); int free(void*); int fill(void*, int byte, size_t, Stream);
//   int sync(Stream); void clear_error(); const char* error_string(int)        (0 = success)
#pragma once
#include "../../include/ekfslam.h"

#include <cstddef>
#include <initializer_list>
#include <string>
#include <vector>

namespace ekfrt {

inline thread_local std::string g_err;

inline ekf_status fail(ekf_status st, const std::string& msg) {
    g_err = msg;
    return st;
}

enum class Fill { kNone = -1, kZero = 0x00, kOnes = 0xFF };   // a byte value, issued on the stream behind the allocation

struct MemTarget { void** p; size_t bytes; Fill fill; };
template <class T>
MemTarget target_bytes(T** p, size_t bytes, Fill fill = Fill::kNone) { return {reinterpret_cast<void**>(p), bytes, fill}; }
template <class T>
MemTarget target(T** p, size_t count, Fill fill = Fill::kNone) { return target_bytes(p, count * sizeof(T), fill); }

template <class Mem>
struct DeviceLedger {
    struct Entry { void* p; size_t bytes; };
    std::vector<Entry> table;
    typename Mem::Stream stream{};   // where the fills go; a pool or handle sets it when its stream exists

    // every failure: the API's last error is cleared, NOMEM for out-of-memory and HIP for anything else
    static ekf_status refuse(int e, const char* fn, const char* what) {
        Mem::clear_error();
        return fail(e == Mem::kOutOfMemory ? EKF_ERR_NOMEM : EKF_ERR_HIP,
                    std::string(fn) + ": " + Mem::error_string(e) + " while reserving " + what);
    }
    size_t bytes() const {
        size_t sum = 0;
        for (const Entry& en : table) sum += en.bytes;
        return sum;
    }
    size_t bytes_of(const void* p) const {
        for (const Entry& en : table) if (en.p == p) return en.bytes;
        return 0;
    }

    // All targets released, then all allocated and filled into locals and committed together; on a failure the locals are
    // freed (behind a synchronisation: fills may be in flight) and every target stays null.
    ekf_status replace_group(std::initializer_list<MemTarget> group, const char* fn, const char* what) {
        for (const MemTarget& t : group) free(t.p);
        std::vector<void*> fresh;
        fresh.reserve(group.size());
        for (const MemTarget& t : group) {
            void* q = nullptr;
            int e = Mem::alloc(&q, t.bytes);
            if (e == 0) {
                fresh.push_back(q);
                if (t.fill != Fill::kNone) e = Mem::fill(q, (int)t.fill, t.bytes, stream);
            }
            if (e != 0) {
                if (!fresh.empty()) (void)Mem::sync(stream);
                for (void* f : fresh) (void)Mem::free(f);
                return refuse(e, fn, what);
            }
        }
        size_t i = 0;
        for (const MemTarget& t : group) {
            *t.p = fresh[i++];
            table.push_back({*t.p, t.bytes});
        }
        return EKF_OK;
    }
    // *p must be null; set only on success
    template <class T>
    ekf_status alloc(T** p, size_t count, Fill fill, const char* fn, const char* what) {
        return replace_group({target(p, count, fill)}, fn, what);
    }
    // Nothing happens when the buffer is large enough already.  Otherwise the new one is allocated and filled into a local;
    // then the old one is freed (which synchronises) and *p changes.  On failure *p and the old buffer are untouched.
    // Contents are not carried over.
    template <class T>
    ekf_status grow(T** p, size_t count, Fill fill, const char* fn, const char* what) {
        if (count * sizeof(T) <= bytes_of(*p)) return EKF_OK;
        T* fresh = nullptr;
        const ekf_status st = alloc(&fresh, count, fill, fn, what);
        if (st != EKF_OK) return st;
        free(p);
        *p = fresh;
        return EKF_OK;
    }
    template <class T>
    void free(T** p) {
        for (size_t i = 0; i < table.size(); i++)
            if (*p && table[i].p == (void*)*p) {
                (void)Mem::free(table[i].p);
                table.erase(table.begin() + i);
                break;
            }
        *p = nullptr;
    }
    void free_all() {
        for (const Entry& en : table) (void)Mem::free(en.p);
        table.clear();
    }
};

// the temporaries of one call: everything goes when the scope ends, whichever return ends it
template <class Mem>
struct ScopedLedger : DeviceLedger<Mem> {
    ScopedLedger() = default;
    explicit ScopedLedger(typename Mem::Stream s) { this->stream = s; }
    ScopedLedger(const ScopedLedger&) = delete;
    ScopedLedger& operator=(const ScopedLedger&) = delete;
    ~ScopedLedger() { this->free_all(); }
};

// A device buffer that is allocated on first use and grows (DeviceLedger::grow), drawn from the ledger it is given.
struct DeviceBuf {
    void* p = nullptr;
    size_t bytes = 0;
    template <class T> T* as() const { return static_cast<T*>(p); }
    template <class Ledger>
    ekf_status reserve(Ledger& mem, size_t need, bool zero_fill, const char* fn, const char* what) {
        if (need <= bytes) return EKF_OK;
        char* q = static_cast<char*>(p);
        const ekf_status st = mem.grow(&q, need, zero_fill ? Fill::kZero : Fill::kNone, fn, what);
        if (st != EKF_OK) return st;
        p = q;
        bytes = need;
        return EKF_OK;
    }
};

}  // namespace ekfrt
