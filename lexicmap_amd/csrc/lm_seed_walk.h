// lm_seed_walk.h — from a seed's number in the packed image back to its list and its anchor partition: the index arithmetic of
// k_sp_dump_range (lm_seedpack.hip), which decodes a range of a resident index's seeds into the (mask, k-mer, value) staging
// form for lm_index_builder_extend.  Free of HIP, so that it is tested on the host against a plain loop
// (tests/seed_walk_host.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LM_SW_HD __host__ __device__ __forceinline__
#else
#define LM_SW_HD inline
#endif

namespace lm {

// The largest l in [lo, hi] with off[l] <= i; off ascending, off[lo] <= i.  With `off` the first-seed table of the lists
// (md_off, out_off: [n + 1]) or a part_tab row ([P + 1]) this is the list / partition that HOLDS seed i: of a run of empty
// ones, which all start where the holder starts, it is the last.
template <typename T> LM_SW_HD int64_t sw_last_le(const T *off, int64_t lo, int64_t hi, int64_t i) {
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// A tile of consecutive seeds [t0, t1] (inclusive) of the piece whose lists are [l0, l1): the tile's first and last list,
// found once per tile - a lane then searches [*lf, *ll] only, which is one list wherever lists are longer than a tile.
LM_SW_HD void sw_tile_lists(const int64_t *off, int64_t l0, int64_t l1, int64_t t0, int64_t t1, int64_t *lf, int64_t *ll) {
    *lf = sw_last_le(off, l0, l1 - 1, t0);
    *ll = sw_last_le(off, *lf, l1 - 1, t1);
}

// The partition of seed `rel` (relative to its list) in the list's part_tab row of P partitions, searched between the
// brackets the tile gives: a seed of the tile's first list lies at or behind the partition of the tile's first seed (pf), a
// seed of its last list at or before the partition of the tile's last seed (pl) - consecutive seeds only move forward.
LM_SW_HD int sw_partition(const uint32_t *row, int P, int64_t rel, bool in_first, int pf, bool in_last, int pl) {
    return (int)sw_last_le(row, in_first ? pf : 0, in_last ? pl : P - 1, rel);
}

// The lists [*l0, *l1) that hold the seeds [s0, s1) of a table off[0 .. n] (s0 < s1 <= off[n]): the host's cut of a piece.
inline void sw_piece_lists(const int64_t *off, int64_t n, int64_t s0, int64_t s1, int64_t *l0, int64_t *l1) {
    *l0 = sw_last_le(off, 0, n - 1, s0);
    *l1 = sw_last_le(off, *l0, n - 1, s1 - 1) + 1;
}

} // namespace lm
