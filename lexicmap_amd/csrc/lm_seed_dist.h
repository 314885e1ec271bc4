// lm_seed_dist.h — the distance between consecutive seeds of a genome record: the rule of lm_index_seed_distances
// (k_sd_pass, lm_seedpack.hip), which is what `lexicmap utils seed-pos` prints (seed-pos.go:385-457) without its flag bit.
// Free of HIP, so that it is tested on the host against a plain loop (tests/seed_dist_host.cpp).
//
// A record's contigs start at s_0 = 0, s_{c+1} = s_c + len_c + contig_interval.  A position p (0-based, in the record's
// concatenation) belongs to the last contig with s_c <= p.  Walking the record's positions in ascending order, the first
// position of a contig has dist = p - s_c and every other one dist = p - the position before it; a contig without seeds
// contributes nothing; a position given twice has dist = 0 the second time.  A position is reported when dist >= min_dist.
// A run of N inside a contig counts as sequence (a resident index stores N as A and keeps no skip regions).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LM_SD_HD __host__ __device__ __forceinline__
#else
#define LM_SD_HD inline
#endif

namespace lm {

// contig starts of a record from its contig lengths: starts[c] for c in [0, n)
inline void sd_contig_starts(const int32_t *len, int32_t n, int32_t contig_interval, uint32_t *starts) {
    uint32_t s = 0;
    for (int32_t c = 0; c < n; c++) {
        starts[c] = s;
        s += (uint32_t)len[c] + (uint32_t)contig_interval;
    }
}

// the last c in [0, n) with starts[c] <= p (starts ascending, starts[0] = 0, n >= 1)
LM_SD_HD int32_t sd_contig(const uint32_t *starts, int32_t n, uint32_t p) {
    int32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int32_t mid = (lo + hi + 1) >> 1;
        if (starts[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

struct SdEntry {
    int32_t contig;  // of the position
    uint32_t start;  // s_c of that contig
    uint32_t dist;
    bool first;      // the first position of its contig
};

// One entry of a record's ascending position list.  has_prev: the list has an entry before this one (of the same record),
// prev_p its position (<= p).  The entry before lies in the same contig exactly when prev_p >= s_c.
LM_SD_HD SdEntry sd_entry(const uint32_t *starts, int32_t n, uint32_t p, bool has_prev, uint32_t prev_p) {
    SdEntry e;
    e.contig = sd_contig(starts, n, p);
    e.start = starts[e.contig];
    e.first = !(has_prev && prev_p >= e.start);
    e.dist = e.first ? p - e.start : p - prev_p;
    return e;
}

LM_SD_HD bool sd_reported(uint32_t dist, uint32_t min_dist) { return dist >= min_dist; }

// histogram counter of a distance: `bins` counters of `width`, the last one taking everything beyond (bins, width >= 1)
LM_SD_HD uint32_t sd_bin(uint32_t dist, uint32_t bins, uint32_t width) {
    const uint32_t b = dist / width;
    return b < bins ? b : bins - 1;
}

} // namespace lm
