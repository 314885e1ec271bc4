// lm_lookup_dev.h — the device helpers of a seed lookup that more than one file needs (lm_kernels.hip: the read search;
// lm_screen.hip: genome screening): the record a stored value belongs to, the genome whitelist, the k-mer range of a prefix
// search.  Device code only.
#pragma once
#include "lm_kernels.h"

namespace lm {

#define LM_LK_OUTLIER_BIT 31
__device__ __forceinline__ int local_genome(const DevIndexView &ix, uint64_t bg) {
    uint64_t batch = bg >> 17, gi = bg & 0x1ffff;
    if (batch >= (uint64_t)ix.nbatches) return -1;
    int64_t g = ix.batch_first[batch] + (int64_t)gi;
    if (ix.g2local) return g < ix.batch_first[ix.nbatches] ? ix.g2local[g] : -1; // chunk-aware shard table (loader)
    if (ix.shard_count > 1) {
        if ((int)(g % ix.shard_count) != ix.shard_rank) return -1;
        g /= ix.shard_count;
    }
    if (g >= ix.ngenomes) return -1;
    return (int)g;
}
__device__ __forceinline__ bool genome_kept(const DevIndexView &ix, int64_t g) {
    return g >= 0 && ((ix.g_keep[g >> 5] >> (g & 31)) & 1u) != 0;
}
__device__ __forceinline__ void lookup_range(uint64_t key, int K, int min_prefix, uint64_t *left, uint64_t *right) {
    if (min_prefix < K) {
        const uint64_t low = (1ull << ((K - min_prefix) << 1)) - 1;
        *left = key & ~low;
        *right = key | low;
    } else {
        *left = *right = key;
    }
}

} // namespace lm
