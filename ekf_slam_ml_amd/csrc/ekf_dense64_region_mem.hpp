// ekf_dense64_region_mem.hpp -- the device memory of a local region (host only, nothing from HIP): the accumulators and the
// scratch of the global update as ONE all-or-nothing group of a ledger (ekf_device_mem.hpp), kept for the next region that
// needs no more.  A template over the ledger so that tests/cpp/region_mem_check.cpp runs it on a recording fake policy.
#pragma once
#include "ekf_dense64_region.hpp"
#include "ekf_device_mem.hpp"

namespace ekfrt {

struct RegionMem {
    void* acc = nullptr;       // Dense64RegionPlan::acc_bytes
    void* scratch = nullptr;   // Dense64RegionPlan::scratch_bytes
    size_t held = 0;           // the two buffers' bytes together, 0 without them

    // Nothing happens when both buffers are large enough.  Otherwise BOTH new ones are allocated into locals first (one
    // group: a failure of either frees the other, and the ledger clears the API's error); only then are the old ones freed
    // and the members changed.  On failure acc, scratch, held and the ledger's table are exactly as they were.
    template <class Ledger>
    ekf_status reserve(Ledger& mem, const ekf::Dense64RegionPlan& pl, const char* fn) {
        if (pl.acc_bytes <= mem.bytes_of(acc) && pl.scratch_bytes <= mem.bytes_of(scratch)) return EKF_OK;
        void *a = nullptr, *s = nullptr;
        const ekf_status st = mem.replace_group({target_bytes(&a, pl.acc_bytes), target_bytes(&s, pl.scratch_bytes)}, fn,
                                                "the region's accumulators and scratch");
        if (st != EKF_OK) return st;
        mem.free(&acc);
        mem.free(&scratch);
        acc = a, scratch = s, held = pl.acc_bytes + pl.scratch_bytes;
        return EKF_OK;
    }
};

}  // namespace ekfrt
