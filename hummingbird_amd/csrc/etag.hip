// etag.hip — md5_etag: the MD5 of the object bytes of a plan's objects where
// they lie in the data shards, one LANE per chain (etag.h).  An object's bytes
// are data shards 0..k-1 of each of its stripes back to back, cut at its length
// (ecGlue, ecutils.go:171-183), and its ETag is their MD5 (ecengine.go:320-321).
// The compression is md5_device.h's and the schedule md5_files' (hashfiles.hip):
// a wave-uniform trip count from the wave's longest chain, two load groups of
// HBEC_MD5_DEPTH_LIST blocks ping-ponged, a load cursor running ahead of a
// compress cursor that takes the same steps, dword-aligned 16-B loads shifted
// into place with v_alignbyte_b32, a bytewise gather only for a block that
// straddles two segments, lanes past their own end keeping their state with a
// select.
//
// What differs is the segment walk.  A cursor stands on {entry, next data shard,
// address, bytes left}; an entry contributes lens[entry] bytes and not its
// shards' whole length, so a chain ends at its own total.  On slot records a run
// of present data shards is one segment (they lie back to back), on row records
// each shard is one; the span of an entry the call decoded beforehand is one
// segment in scratch on both (etag_segment_slot, etag_segment_rows).  A healthy
// entry of a stripe plan is one segment, so the only straddling blocks are the
// ones at entry boundaries.
//
// The filter is read on the device: a lane scans its object's entries for a
// passing word before any shard load, and a wave with no examined lane returns.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "etag.h"
#include "gf_device.h"
#include "hashplan.h"
#include "kernels.h"
#include "md5_device.h"

namespace hbec {

namespace {

// load target of straddling blocks and of lanes past their end
__device__ __attribute__((aligned(16))) uint8_t kEtagZeroBlock[64];

typedef __attribute__((address_space(1))) const uint32_t eu32_c;
typedef __attribute__((address_space(1))) const uint8_t eu8_c;
typedef __attribute__((address_space(1))) const uint64_t eu64_c;
// 16 B at a dword-aligned address: one global_load_dwordx4
typedef uint32_t eu32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) const eu32x4_a4 eu32x4_a4_c;

// Where a lane stands in its chain: on byte `addr` of a segment of entry `e`
// with `left` bytes to go; the entry's next segment starts at data shard `j`.
struct ECursor {
    uint32_t e, j;
    uint64_t addr, left;
};

}  // namespace

#define HBEC_ETAG_KERNEL md5_etag
#define HBEC_ETAG_ROWS 0
#include "etag_kernel.inc"
#undef HBEC_ETAG_KERNEL
#undef HBEC_ETAG_ROWS

// md5_etag over a shards plan's records
#define HBEC_ETAG_KERNEL md5_etag_rows
#define HBEC_ETAG_ROWS 1
#include "etag_kernel.inc"
#undef HBEC_ETAG_KERNEL
#undef HBEC_ETAG_ROWS

int launch_etag_chains(const void* recs, const ERec* erecs, const EChain* chains, uint64_t n_chains, int k,
                       const uint32_t* filter, uint32_t filter_bits, const uint8_t* expected, uint8_t* digests,
                       uint32_t* bad, void* stream, bool rows) {
    if (n_chains == 0) return (int)hipSuccess;
    const dim3 grid((unsigned)((n_chains + 63) / 64));
    auto* kernel = rows ? &md5_etag_rows : &md5_etag;
    hipLaunchKernelGGL(kernel, grid, dim3(64), 0, static_cast<hipStream_t>(stream), static_cast<const HRec*>(recs),
                       erecs, chains, n_chains, (uint32_t)k, filter, filter_bits, expected, digests, bad);
    return (int)hipGetLastError();
}

}  // namespace hbec
