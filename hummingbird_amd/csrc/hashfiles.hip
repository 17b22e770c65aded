// hashfiles.hip — md5_files: the ShardHash of the selected shard FILES of a
// plan's objects, one LANE per chain (hashfiles.h).  A shard file is shard j of
// each of the object's entries back to back (ecSplit appends it stripe by
// stripe, ecutils.go:38-70), hashed as one stream: one pad, one 64-bit length.
// The compression is md5_device.h's and the schedule md5_plan's (hashplan.hip):
// a wave-uniform trip count from the wave's longest chain, counted in blocks of
// the TOTAL length, two load groups of HBEC_MD5_DEPTH_LIST blocks ping-ponged,
// lanes past their own end keeping their state with a select.
//
// What differs is that a lane walks a list of segments, not one address.  It
// keeps two cursors {entry, address, bytes left in the segment}: one for the
// loads running ahead, one for the block being compressed.  Both take the same
// steps, so the block a slot was loaded for is the block the other cursor
// stands on when the slot is compressed.  A 64-B block that lies wholly inside
// a segment takes md5_plan's loader: dword-aligned 16-B groups from addr & ~3
// plus one dword, shifted into place with 16 v_alignbyte_b32.  The shift comes
// from that block's own address, since it changes at every segment boundary and
// after every block that straddles one; shift 0 re-reads the block's last dword,
// so no load touches a dword that holds no byte of the segment.  A block that
// straddles a boundary (a short last piece, or pieces so small that one block
// spans three or more of them) is put together bytewise from the segments it
// spans, in a branch a wave enters only when one of its lanes needs it; its
// prefetch slot loads the zero block.  So do the slots of lanes past their end.
//
// The filter is read on the device: a lane scans its object's entries for a
// passing word before any shard load (a shard file can only be hashed whole),
// and a wave with no examined lane returns at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gf_device.h"
#include "hashfiles.h"
#include "kernels.h"
#include "md5_device.h"

namespace hbec {

namespace {

// load target of straddling blocks and of lanes past their end
__device__ __attribute__((aligned(16))) uint8_t kFilesZeroBlock[64];

typedef __attribute__((address_space(1))) const uint32_t fu32_c;
typedef __attribute__((address_space(1))) const uint8_t fu8_c;
typedef __attribute__((address_space(1))) const uint64_t fu64_c;
// 16 B at a dword-aligned address: one global_load_dwordx4
typedef uint32_t fu32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef __attribute__((address_space(1))) const fu32x4_a4 fu32x4_a4_c;

// Where a lane stands in its chain: on byte `addr` of entry `e`'s shard, with
// `left` bytes of that shard to go.
struct FCursor {
    uint32_t e;
    uint64_t addr, left;
};

}  // namespace

#define HBEC_MD5_FILES_KERNEL md5_files
#define HBEC_MD5_FILES_ROWS 0
#include "hashfiles_kernel.inc"
#undef HBEC_MD5_FILES_KERNEL
#undef HBEC_MD5_FILES_ROWS

// md5_files over a shards plan's records
#define HBEC_MD5_FILES_KERNEL md5_files_rows
#define HBEC_MD5_FILES_ROWS 1
#include "hashfiles_kernel.inc"
#undef HBEC_MD5_FILES_KERNEL
#undef HBEC_MD5_FILES_ROWS

__global__ __launch_bounds__(256) void hash_files_where(const HRec* __restrict__ recs, uint32_t n_src,
                                                        const uint32_t* __restrict__ object_of,
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
        const uint32_t g = object_of[i];
        w = hash_where_word(sel[g], bad[g], r.route);
    }
    if (w) atomicOr(where + i, w);
}

hipError_t launch_md5_files(const HRec* recs, const uint32_t* object_start, const FChain* chains, uint64_t n_chains,
                            int k, int n, const uint32_t* filter, uint32_t filter_bits, const uint8_t* expected,
                            uint8_t* digests, uint32_t* bad, hipStream_t stream, bool rows) {
    if (n_chains == 0) return hipSuccess;
    const dim3 grid((unsigned)((n_chains + 63) / 64));
    hipLaunchKernelGGL(rows ? md5_files_rows : md5_files, grid, dim3(64), 0, stream, recs, object_start, chains,
                       n_chains, (uint32_t)k, (uint32_t)n, filter, filter_bits, expected, digests, bad);
    return hipGetLastError();
}

hipError_t launch_hash_files_where(const HRec* recs, uint32_t n_src, const uint32_t* object_of, const uint32_t* sel,
                                   const uint32_t* filter, uint32_t filter_bits, const uint32_t* bad, uint32_t* where,
                                   hipStream_t stream) {
    if (n_src == 0) return hipSuccess;
    const dim3 grid((unsigned)(((uint64_t)n_src + 255) / 256));
    hipLaunchKernelGGL(hash_files_where, grid, dim3(256), 0, stream, recs, n_src, object_of, sel, filter, filter_bits,
                       bad, where);
    return hipGetLastError();
}

}  // namespace hbec
