// lm_merge.h - the shard merge on the device (lm_merge.hip), used by lm_gather_merge_rows (lm_comm.cpp)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/lexicmap_hip.h"

namespace lm {
// The string columns (cigar, qseq, sseq, align) on the wire (lm_gather_rows_ex and kin, include/lexicmap_hip.h): per row four
// uint32 lengths (kStrNull = a NULL string) and one block `cigar\0qseq\0sseq\0align\0` - a NULL string takes no byte - zero-padded
// to a multiple of 16 bytes, the blocks of the rows back to back in row order.  A row of four NULL strings has an empty block.
constexpr uint32_t kStrNull = 0xFFFFFFFFu;
__host__ __device__ inline uint64_t str_bytes(uint32_t len) { return len == kStrNull ? 0 : (uint64_t)len + 1; }
__host__ __device__ inline uint64_t block_bytes(const uint32_t *len4) {
    const uint64_t s = str_bytes(len4[0]) + str_bytes(len4[1]) + str_bytes(len4[2]) + str_bytes(len4[3]);
    return (s + 15) & ~(uint64_t)15;
}

struct MergeScratch { // grow-only device buffers, owned by the communicator
    void *head = nullptr, *gid = nullptr, *sim = nullptr, *keys = nullptr, *keys2 = nullptr, *first = nullptr, *cnt = nullptr, *sizes = nullptr,
         *hits = nullptr, *outpos = nullptr, *tmp = nullptr, *off = nullptr;
    void *src = nullptr, *soff = nullptr, *doff = nullptr, *xend = nullptr; // the string columns' reordering (MergeStrings)
    size_t cap[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    // Set for the duration of ONE call when the merging rank's index handle is known: the buffers are then borrowed from the
    // handle's scratch slabs - idle between two searches - and given back at the end, instead of hipMalloc'ed beside them (a
    // production-size handle holds 72 % of the device in its lane slabs: at shard-of-4 the 2.5 GB of the merge did not fit).
    void *(*borrow)(void *ctx, size_t bytes) = nullptr;
    void (*give_back)(void *ctx, void *p) = nullptr;
    void *ctx = nullptr;
    void *borrowed[32];
    int nborrowed = 0;
    void *take(size_t bytes); // one buffer for this call (borrow mode only)
    void end_call();          // give everything borrowed back, forget the pointers
    void release();
};
// The string columns of a merge: in = the lengths (4 per row) and the blocks of the input rows, rank order like the rows (wire form
// above); out = `bytes` of device memory for the blocks in output order; host = the address the output rows' cigar / qseq / sseq /
// align are written against (the pinned buffer the blocks are downloaded into, same layout).
struct MergeStrings {
    const uint32_t *lens = nullptr;
    const char *in = nullptr;
    char *out = nullptr;
    uint64_t bytes = 0;
    uint64_t host = 0;
};
// str == NULL: the rows only, pointer columns cleared.  str != NULL: the blocks follow their rows; hipErrorInvalidValue when the
// lengths do not add up to str->bytes (nothing is copied then).
hipError_t merge_rows_device(hipStream_t st, const lm_hsp *d_rows, size_t n, const int64_t *off_host, int nranks, lm_hsp *d_out, MergeScratch &S,
                             const MergeStrings *str = nullptr);
} // namespace lm

struct lm_index;
// genome_id / seq_id of rows that came from other processes (lm_pipeline.hip): every shard holds the names of all genomes; the
// names of a synthetic set are made once per genome and kept with the handle.  Threaded over the rows.
extern "C" void lm_attach_names(lm_index *ix, lm_hsp *rows, size_t n); // (internal: not in the public header)
// The handle's scratch slabs lent to the caller between two searches (lm_pipeline.hip; internal).  begin takes the handle's
// mutex - no search can start meanwhile - end releases it; borrow returns NULL when the scratch cannot hold the block.
extern "C" void lm_scratch_session_begin(lm_index *ix);
extern "C" void lm_scratch_session_end(lm_index *ix);
extern "C" void *lm_scratch_borrow(lm_index *ix, size_t bytes);
extern "C" void lm_scratch_return(lm_index *ix, void *p);
