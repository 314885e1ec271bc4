// lm_lookup_dev.h — the device helpers of a seed lookup that more than one file needs (lm_kernels.hip: the read search;
// lm_screen.hip: genome screening): the record a stored value belongs to, the genome whitelist, the k-mer range of a prefix
// search, the reference's start rule.  Device code only.
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

// The reference finds the start of a search through the anchor index of a mask's list (kv-reader.go:762-1021 builds it while
// it reads, kv-searcher2.go:326-549 uses it): index[anchor] = where a run of consecutive k-mers with these a anchor bases
// begins in the list - ALL seeds of the mask, normal and reversed, sorted by k-mer - and a LATER run with the same anchor bases
// overwrites an earlier one.  In a list whose k-mers all start with the mask's prefix every anchor has one run.  A list that
// also holds k-mers of other prefixes (the captures of genomes without the mask's prefix: tiny genomes) can hold a second
// run, and then a search for a k-mer of the earlier run starts behind its range and returns nothing.  So: walking the list
// upwards from the searched range, k-mers with the range's anchor continue its run until one with another anchor ends it; one
// more k-mer with that anchor afterwards and the lookup is empty.  Here the list is four sorted pieces - the packed partitions
// and the flat outliers of both directions; the partitions share the mask's prefix, so they are one stretch of the walk and
// the partition table says whether it holds anchors below, at and above the range's.
// A shard holds the seeds of its own records only, so its lists are not the index's lists.  ScreenShadowTab is the part of
// ALL shards' lists this walk reads - per list the occupied partitions as a bitmap (W words, `sum`: which words are not 0)
// and the outlier k-mers, without values - put together by lm_index_screen_add_structure from what
// lm_index_screen_structure exports of every shard; bits == null: the handle's own lists are the index's.
__device__ inline bool screen_shadowed(const DevIndexView &ix, const ScreenShadowTab &T, uint32_t m, uint64_t x, uint64_t right) {
    const uint64_t *out_kmers = T.bits ? T.kmers : ix.out_kmers;
    const int64_t *out_off = T.bits ? T.off : ix.out_off;
    const int sh = (ix.K - ix.mask_prefix) << 1;
    const uint64_t am = (uint64_t)(ix.P1 - 2);
    const uint64_t A = (x >> ix.key_bits) & am, tx = x >> sh, mp = ix.masks[m] >> sh;
    bool m_less = false, m_at = false, m_more = false;
    int64_t at[2], end[2];
    for (int dir = 0; dir < 2; dir++) {
        if (T.bits) {
            const int64_t md = 2 * (int64_t)m + dir;
            const int w = (int)(A >> 6), b = (int)(A & 63);
            const uint64_t word = T.bits[md * T.W + w], sum = T.sum[md];
            m_less |= (sum & ((1ull << w) - 1)) != 0 || (word & ((1ull << b) - 1)) != 0;
            m_at |= ((word >> b) & 1ull) != 0;
            m_more |= (w < 63 && (sum >> (w + 1)) != 0) || (b < 63 && (word >> (b + 1)) != 0);
        } else {
            const uint32_t *row = ix.part_tab + (int64_t)(2 * m + dir) * ix.P1;
            m_less |= row[A] > row[0];
            m_at |= row[A + 1] > row[A];
            m_more |= row[ix.P1 - 1] > row[A + 1];
        }
        int64_t lo = out_off[2 * m + dir], hi = out_off[2 * m + dir + 1];
        end[dir] = hi;
        while (lo < hi) { // the first outlier above the range
            const int64_t mid = (lo + hi) >> 1;
            if (out_kmers[mid] <= right) lo = mid + 1;
            else hi = mid;
        }
        at[dir] = lo;
    }
    bool ended = false, main_done = tx > mp;
    if (tx == mp) { // the range lies in the partitions: what follows it there, then the outliers above
        ended = m_more;
        main_done = true;
    }
    for (;;) {
        const bool h0 = at[0] < end[0], h1 = at[1] < end[1];
        uint64_t y = 0;
        int from = -1;
        if (h0) {
            y = out_kmers[at[0]];
            from = 0;
        }
        if (h1 && (!h0 || out_kmers[at[1]] < y)) {
            y = out_kmers[at[1]];
            from = 1;
        }
        if (!main_done && (from < 0 || (y >> sh) > mp)) { // the partitions come first
            if (m_less) ended = true;
            if (m_at && ended) return true;
            if (m_more) ended = true;
            main_done = true;
            continue;
        }
        if (from < 0) return false;
        if (((y >> ix.key_bits) & am) == A) {
            if (ended) return true;
        } else {
            ended = true;
        }
        at[from]++;
    }
}

} // namespace lm
