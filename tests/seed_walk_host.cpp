// Host build of the seed-number -> list / partition arithmetic of k_sp_dump_range (lexicmap_amd/csrc/lm_seed_walk.h) for
// tests/test_extend_index_cpu.py: a piece of the image is walked tile by tile exactly as the kernel's workgroups walk it.
#include "../lexicmap_amd/csrc/lm_seed_walk.h"

using namespace lm;

extern "C" {

// seeds [s0, s1) of an image with n lists (off[n + 1]) and P partitions per list (tab[n][P + 1], relative to the list's first
// seed), in tiles of `tile` seeds: list and partition of every seed to out_list / out_part[i - s0]
void sw_walk(const int64_t *off, const uint32_t *tab, int64_t n, int P, int64_t s0, int64_t s1, int tile, int32_t *out_list, int32_t *out_part) {
    int64_t l0, l1;
    sw_piece_lists(off, n, s0, s1, &l0, &l1);
    for (int64_t t0 = s0; t0 < s1; t0 += tile) {
        const int64_t t1 = (t0 + tile < s1 ? t0 + tile : s1) - 1;
        int64_t lf, ll;
        sw_tile_lists(off, l0, l1, t0, t1, &lf, &ll);
        const int pf = (int)sw_last_le(tab + lf * (P + 1), 0, P - 1, t0 - off[lf]);
        const int pl = (int)sw_last_le(tab + ll * (P + 1), lf == ll ? pf : 0, P - 1, t1 - off[ll]);
        for (int64_t i = t0; i <= t1; i++) {
            const int64_t md = sw_last_le(off, lf, ll, i);
            out_list[i - s0] = (int32_t)md;
            out_part[i - s0] = sw_partition(tab + md * (P + 1), P, i - off[md], md == lf, pf, md == ll, pl);
        }
    }
}
void sw_lists_of_piece(const int64_t *off, int64_t n, int64_t s0, int64_t s1, int64_t *l0, int64_t *l1) { sw_piece_lists(off, n, s0, s1, l0, l1); }
}
