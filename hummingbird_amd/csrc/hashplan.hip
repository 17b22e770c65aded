// hashplan.hip — md5_plan: the ShardHash of the selected shards of a plan, one
// LANE per chain (hashplan.h).  The compression and the schedule are md5_list's
// (md5.hip): a wave-uniform trip count from the wave's longest chain, two load
// groups of HBEC_MD5_DEPTH_LIST blocks ping-ponged, lanes past their own end
// loading clamped blocks and keeping their state with a select.
//
// What differs is how a lane reaches its bytes.  In a plan 15 object sizes in 16
// put shards at odd addresses (ecutils.go:14-24,31-35), and the lanes of a wave
// sit at different residues.  Each lane loads dword-aligned 16-B groups from
// addr & ~3 plus the dword after them, and shifts neighbouring dwords into place
// with v_alignbyte_b32, its own addr & 3 as the shift: 17 loaded dwords and 16
// shifts per 64-B block.  (md5_list's byte loader is no 64 byte loads in the code
// object: the compiler merges them into 16-B loads at byte addresses, whose
// split line accesses cost 8 % of the call once waves share a CU, and nothing
// while each wave has a CU's load path to itself)
// A lane with shift 0 gets its loads back unchanged and its extra dword
// is the block's last one again, so no load touches a dword that holds no byte
// of the lane's shard: with shift s > 0 the dword after block b holds the
// block's last s bytes.  The tail of fewer than 64 bytes is read bytewise.
//
// The filter is read on the device: a lane whose entry is not examined is an
// empty chain, and a wave with no examined lane returns before any shard load.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "hashplan.h"
#include "kernels.h"
#include "md5_device.h"

#ifndef HBEC_HASH_PLAN_BYTE_LOADER
// 0 = dword-aligned 16-B loads shifted into place per lane; 1 = md5_list's byte
// loader, which the compiler merges into 16-B loads at byte addresses: the A/B
// partner of profiles/hash_plan.jsonl
#define HBEC_HASH_PLAN_BYTE_LOADER 0
#endif

namespace hbec {

__device__ __attribute__((aligned(16))) uint8_t kHashZeroBlock[64];  // load target of empty chains

typedef __attribute__((address_space(1))) const uint32_t gu32_c;
// 16 B at a dword-aligned address: one global_load_dwordx4
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) const u32x4_a4 gu32x4_a4_c;

typedef __attribute__((address_space(1))) const uint64_t gu64_c;

#define HBEC_MD5_PLAN_KERNEL md5_plan
#define HBEC_MD5_PLAN_ROWS 0
#include "hashplan_kernel.inc"
#undef HBEC_MD5_PLAN_KERNEL
#undef HBEC_MD5_PLAN_ROWS

// md5_plan over a shards plan's records: a lane loads its shard's address from the entry's row
#define HBEC_MD5_PLAN_KERNEL md5_plan_rows
#define HBEC_MD5_PLAN_ROWS 1
#include "hashplan_kernel.inc"
#undef HBEC_MD5_PLAN_KERNEL
#undef HBEC_MD5_PLAN_ROWS

__global__ __launch_bounds__(256) void hash_where(const HRec* __restrict__ recs, uint32_t n_src,
                                                  const uint32_t* __restrict__ sel,
                                                  const uint32_t* __restrict__ filter, uint32_t filter_bits,
                                                  const uint32_t* __restrict__ bad, uint32_t* where) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n_src) return;
    const HRec r = recs[i];
    if (r.len == 0) return;
    uint32_t w = kLocSkipped;  // the other route, filtered or not
    if (r.route == (uint32_t)kVmKernel) {
        if (filter && !(filter[i] & filter_bits)) return;
        w = hash_where_word(sel[i], bad[i], r.route);
    }
    if (w) atomicOr(where + i, w);
}

hipError_t launch_md5_plan(const HRec* recs, const HChain* chains, uint64_t n_chains, int k, int n,
                           const uint32_t* filter, uint32_t filter_bits, const uint8_t* expected, uint8_t* digests,
                           uint32_t* bad, hipStream_t stream, bool rows) {
    if (n_chains == 0) return hipSuccess;
    const dim3 grid((unsigned)((n_chains + 63) / 64));
    hipLaunchKernelGGL(rows ? md5_plan_rows : md5_plan, grid, dim3(64), 0, stream, recs, chains, n_chains, (uint32_t)k,
                       (uint32_t)n, filter, filter_bits, expected, digests, bad);
    return hipGetLastError();
}

hipError_t launch_hash_where(const HRec* recs, uint32_t n_src, const uint32_t* sel, const uint32_t* filter,
                             uint32_t filter_bits, const uint32_t* bad, uint32_t* where, hipStream_t stream) {
    if (n_src == 0) return hipSuccess;
    const dim3 grid((unsigned)(((uint64_t)n_src + 255) / 256));
    hipLaunchKernelGGL(hash_where, grid, dim3(256), 0, stream, recs, n_src, sel, filter, filter_bits, bad, where);
    return hipGetLastError();
}

}  // namespace hbec
