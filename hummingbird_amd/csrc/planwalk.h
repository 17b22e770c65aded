// planwalk.h — the launch of a kernel that walks a plan's static {entry, tile}
// list (mixedplan.h): gf_mixed_plan, gf_verify_mixed_plan, gf_repair_mixed_plan,
// gf_locate_mixed_plan and gf_heal_mixed_plan differ in their arguments alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>

#include "kernels.h"

namespace hbec {

// fn: the instance its file picked (nullptr: no instance for that r); occ: that
// instance's blocks per CU, asked once; K <= kOddMaxK inputs.  One wave per
// tile, as many blocks as fit the device at most.
inline hipError_t launch_plan_walk(const void* fn, std::atomic<int>* occ, int k, uint32_t n_tiles, int cus,
                                   void** args, hipStream_t stream) {
    if (!fn || k < 1 || k > kOddMaxK || cus < 1) return hipErrorInvalidValue;
    if (n_tiles == 0) return hipSuccess;
    int per_cu = occ->load(std::memory_order_relaxed);
    if (per_cu == 0) {
        hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlockThreads, 0);
        if (e != hipSuccess) return e;
        occ->store(std::max(1, per_cu), std::memory_order_relaxed);
    }
    constexpr uint64_t wpb = kBlockThreads / 64;
    const uint64_t grid =
        std::max<uint64_t>(1, std::min<uint64_t>((n_tiles + wpb - 1) / wpb, (uint64_t)cus * std::max(1, per_cu)));
    return hipLaunchKernel(fn, dim3((uint32_t)grid), dim3(kBlockThreads), args, 0, stream);
}

}  // namespace hbec
