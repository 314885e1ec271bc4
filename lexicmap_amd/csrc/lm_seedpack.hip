// lm_seedpack.hip — construction of the packed seed image in HBM (DevIndexView).
//
// Replaces the 16 B/seed RAM form of the reference (kv-reader.go:762-1021: per mask a flat []uint64{kmer, value, ...} plus a
// 4^a-entry first-offset table) by, per list md = (mask, direction):
//     part_tab[md][4^a + 1]   u32 offsets of the anchor partitions (the a bases after the mask's p-base prefix)
//     pk_keys                 bit stream, 2 (K-p-a) bits per seed: the rest of the k-mer, ascending inside a partition
//     pk_vals                 bit stream, gid_bits + pos_bits + 1 bits per seed: local genome | position | strand
// = 9.5 B/seed for K=31, p=7, a=6 and 100k x 3-Mb genomes per GPU (+ 0.66 GB of table for M=20000), so that BASELINE
// configs 3-5 fit the 288 GB of one MI355X per shard.  Seeds that do not start with their mask's prefix (only possible
// for genomes that lack the prefix, i.e. tiny ones) keep the flat 16-byte form in per-list outlier arrays.
//
// Built in two passes over the seeds, shown in any order and any batching (loader: chunk files; synthetic builder:
// genome chunks): count() -> partition sizes, place() -> atomic slot per partition + atomicOr into the zeroed streams,
// finish() -> every partition sorted by key in place (one wavefront per partition, LDS bitonic network; partitions
// shared words are merged with masked atomics).  No copy of the unpacked seeds ever exists.
#include "lm_prims.h"
#include "lm_seed_dist.h"
#include "lm_seed_walk.h"

#include <errno.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <thread>

namespace lm {

#define SP_MAXN 1024 /* largest partition the LDS sorter takes; beyond: rocPRIM fallback */

struct SpParams {
    const uint64_t *masks;
    int K, p, a, P1, key_bits, gid_bits, pos_bits, M;
    const int64_t *batch_first;
    int nbatches, shard_rank, shard_count;
    const int32_t *g2local;
};

__device__ __forceinline__ int64_t sp_local_genome(const SpParams &sp, uint64_t bg) {
    const uint64_t batch = bg >> 17, gi = bg & 0x1ffff;
    int64_t g = (batch < (uint64_t)sp.nbatches ? sp.batch_first[batch] : 0) + (int64_t)gi;
    if (sp.g2local) return sp.g2local[g];
    if (sp.shard_count > 1) g /= sp.shard_count;
    return g;
}

// returns the table slot (md*P1 + part) of a seed, or -1 - md for an outlier
__device__ __forceinline__ int64_t sp_classify(const SpParams &sp, uint32_t m, uint64_t kmer, uint64_t val) {
    const uint32_t md = (m << 1) | (uint32_t)(val & 1ull);
    const int sh = (sp.K - sp.p) << 1;
    if ((kmer >> sh) != (sp.masks[m] >> sh)) return -1 - (int64_t)md;
    const uint32_t part = (uint32_t)(kmer >> sp.key_bits) & (uint32_t)(sp.P1 - 2);
    return (int64_t)md * sp.P1 + part;
}

__global__ void k_sp_count(SpParams sp, const uint16_t *__restrict__ mask, const uint64_t *__restrict__ kmer,
                           const uint64_t *__restrict__ val, int64_t n, uint32_t *__restrict__ tab,
                           unsigned long long *__restrict__ out_cnt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = sp_classify(sp, mask[i], kmer[i], val[i]);
        if (s >= 0)
            atomicAdd(&tab[s + 1], 1u); // count of partition `part` sits one entry up: see k_sp_scan_rows
        else
            atomicAdd(&out_cnt[-1 - s], 1ull);
    }
}

// per list: counts in row[1..P] -> row[i+1] = first seed of partition i (exclusive scan), row[0] = 0; total -> md_cnt.
// place() then uses row[i+1] as the cursor of partition i, which leaves row[i+1] = first seed of partition i+1: the
// final table needs no second array.
__global__ __launch_bounds__(256) void k_sp_scan_rows(uint32_t *__restrict__ tab, int P1, int64_t nmd,
                                                      unsigned long long *__restrict__ md_cnt) {
    __shared__ uint32_t part_sum[256];
    const int P = P1 - 1;
    const int ipt = (P + 255) / 256;
    for (int64_t md = blockIdx.x; md < nmd; md += gridDim.x) {
        uint32_t *row = tab + md * P1 + 1;
        const int b = threadIdx.x * ipt, e = min(P, b + ipt);
        uint32_t s = 0;
        for (int i = b; i < e; i++) s += row[i];
        part_sum[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t acc = 0;
            for (int t = 0; t < 256; t++) {
                const uint32_t v = part_sum[t];
                part_sum[t] = acc;
                acc += v;
            }
            md_cnt[md] = acc;
        }
        __syncthreads();
        uint32_t acc = part_sum[threadIdx.x];
        for (int i = b; i < e; i++) {
            const uint32_t v = row[i];
            row[i] = acc;
            acc += v;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void sp_bits_or(uint64_t *a, int64_t i, int w, uint64_t v) {
    const int64_t bit = i * (int64_t)w;
    const int64_t word = bit >> 6;
    const int sh = (int)(bit & 63);
    atomicOr((unsigned long long *)&a[word], (unsigned long long)(v << sh));
    if (sh + w > 64) atomicOr((unsigned long long *)&a[word + 1], (unsigned long long)(v >> (64 - sh)));
}

__global__ void k_sp_place(SpParams sp, const uint16_t *__restrict__ mask, const uint64_t *__restrict__ kmer,
                           const uint64_t *__restrict__ val, int64_t n, uint32_t *__restrict__ tab,
                           const int64_t *__restrict__ md_off, uint64_t *__restrict__ pk_keys, uint64_t *__restrict__ pk_vals,
                           const int64_t *__restrict__ out_off, unsigned long long *__restrict__ out_cur,
                           uint64_t *__restrict__ out_kmers, uint64_t *__restrict__ out_vals) {
    const uint64_t km = (1ull << sp.key_bits) - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = kmer[i], v = val[i];
        const int64_t s = sp_classify(sp, mask[i], k, v);
        if (s >= 0) {
            const int64_t md = s / sp.P1;
            const int64_t slot = md_off[md] + (int64_t)atomicAdd(&tab[s + 1], 1u);
            sp_bits_or(pk_keys, slot, sp.key_bits, k & km);
            sp_bits_or(pk_vals, slot, sp.gid_bits + sp.pos_bits + 1,
                       lm_pack_seed_val((uint64_t)sp_local_genome(sp, v >> 30), v, sp.pos_bits));
        } else {
            const int64_t md = -1 - s;
            const int64_t o = out_off[md] + (int64_t)atomicAdd(&out_cur[md], 1ull);
            out_kmers[o] = k;
            out_vals[o] = v;
        }
    }
}

// ---- in-place sort of the partitions -----------------------------------------------------------------------------------
template <typename Get>
__device__ __forceinline__ void sp_store_range(uint64_t *a, int64_t first, int64_t n, int width, Get get, int lane, int nl) {
    const int64_t w0 = (first * width) >> 6, w1 = ((first + n) * width - 1) >> 6;
    for (int64_t w = w0 + lane; w <= w1; w += nl) {
        uint64_t m;
        const uint64_t v = lm_bits_build_word(w, first, n, width, get, &m);
        if (m == ~0ull) {
            a[w] = v;
        } else { // a word shared with the neighbouring partitions: only our bits
            atomicAnd((unsigned long long *)&a[w], (unsigned long long)~m);
            atomicOr((unsigned long long *)&a[w], (unsigned long long)v);
        }
    }
}

// one wavefront per partition; partitions above SP_MAXN go to `big` (list of table slots)
__global__ __launch_bounds__(64) void k_sp_sort_parts(const uint32_t *__restrict__ tab, const int64_t *__restrict__ md_off,
                                                      int P1, int64_t nmd, int key_bits, int val_bits,
                                                      uint64_t *__restrict__ pk_keys, uint64_t *__restrict__ pk_vals,
                                                      unsigned long long *__restrict__ big, unsigned long long big_cap,
                                                      unsigned long long *__restrict__ nbig, int dbg_mode) {
    __shared__ uint64_t sk[SP_MAXN], sv[SP_MAXN];
    const int lane = threadIdx.x;
    const int P = P1 - 1;
    const int64_t nparts = nmd * P;
    for (int64_t pi = blockIdx.x; pi < nparts; pi += gridDim.x) {
        const int64_t md = pi / P, part = pi % P;
        const uint32_t *row = tab + md * P1 + part;
        const int64_t n = (int64_t)row[1] - (int64_t)row[0];
        if (n <= 1) continue;
        const int64_t first = md_off[md] + row[0];
        if (n > SP_MAXN) {
            if (lane == 0) {
                const unsigned long long o = atomicAdd(nbig, 1ull);
                if (o < big_cap) big[o] = (unsigned long long)(md * P1 + part);
            }
            continue;
        }
        int npad = 2;
        while (npad < n) npad <<= 1;
        bool sorted = true;
        for (int i = lane; i < npad; i += 64) {
            if (i < n) {
                sk[i] = lm_bits_get(pk_keys, first + i, key_bits);
                sv[i] = lm_bits_get(pk_vals, first + i, val_bits);
            } else {
                sk[i] = ~0ull;
                sv[i] = ~0ull;
            }
        }
        __syncthreads();
        for (int i = lane; i + 1 < n; i += 64)
            if (sk[i] > sk[i + 1]) sorted = false;
        if (__ballot(!sorted) == 0) { // nothing to do (chunks arrive in key order more often than not)
            __syncthreads();
            continue;
        }
        if (dbg_mode & 1) {
            __syncthreads();
            continue;
        }
        for (int k = 2; k <= ((dbg_mode & 2) ? 1 : npad); k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = lane; i < (npad >> 1); i += 64) {
                    const int x = ((i & ~(j - 1)) << 1) | (i & (j - 1)), y = x | j;
                    const bool up = (x & k) == 0;
                    const uint64_t kx = sk[x], ky = sk[y];
                    if ((kx > ky) == up && kx != ky) {
                        sk[x] = ky;
                        sk[y] = kx;
                        const uint64_t t = sv[x];
                        sv[x] = sv[y];
                        sv[y] = t;
                    }
                }
                __syncthreads();
            }
        }
        if (!(dbg_mode & 4)) {
            sp_store_range(pk_keys, first, n, key_bits, [&](int64_t i) { return sk[i]; }, lane, 64);
            sp_store_range(pk_vals, first, n, val_bits, [&](int64_t i) { return sv[i]; }, lane, 64);
        }
        __syncthreads();
    }
}

// ---- partitions above SP_MAXN seeds ------------------------------------------------------------------------------------
// Every mask has a few of them: the k-mers a mask captures are the ones closest to it, so the captures of ALL genomes under a
// mask share ~log4(genome length) bases with the mask and pile up in the partitions around the mask's own 13-base prefix
// (thousands to 10^5 seeds at 10^4-10^5 genomes).  They are unpacked in batches, sorted by one rocPRIM segmented radix sort
// per batch and packed back.
__global__ void k_sp_big_info(const unsigned long long *__restrict__ slots, int64_t nb, const uint32_t *__restrict__ tab,
                              const int64_t *__restrict__ md_off, int P1, int64_t *__restrict__ first, int64_t *__restrict__ cnt) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long s = slots[i];
        first[i] = md_off[s / P1] + tab[s];
        cnt[i] = (int64_t)tab[s + 1] - (int64_t)tab[s];
    }
}
// element e of the batch = seed (e - off[p]) of big partition p (off relative to the batch)
__global__ void k_sp_unpack_many(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ vals, int key_bits, int val_bits,
                                 const int64_t *__restrict__ first, const int64_t *__restrict__ off, int64_t nseg, int64_t base,
                                 int64_t total, uint64_t *__restrict__ ko, uint64_t *__restrict__ vo) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = nseg; // last p with off[p] - base <= e
        while (lo + 1 < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (off[mid] - base <= e)
                lo = mid;
            else
                hi = mid;
        }
        const int64_t src = first[lo] + (e - (off[lo] - base));
        ko[e] = lm_bits_get(keys, src, key_bits);
        vo[e] = lm_bits_get(vals, src, val_bits);
    }
}
__global__ void k_sp_rel_offsets(const int64_t *__restrict__ off, int64_t nseg, int64_t base, uint32_t *__restrict__ rel) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= nseg; i += (int64_t)gridDim.x * blockDim.x)
        rel[i] = (uint32_t)(off[i] - base);
}
__global__ __launch_bounds__(256) void k_sp_repack_many(uint64_t *__restrict__ keys, uint64_t *__restrict__ vals, int key_bits,
                                                         int val_bits, const int64_t *__restrict__ first,
                                                         const uint32_t *__restrict__ rel, int64_t nseg,
                                                         const uint64_t *__restrict__ ki, const uint64_t *__restrict__ vi) {
    for (int64_t p = blockIdx.x; p < nseg; p += gridDim.x) {
        const int64_t n = (int64_t)rel[p + 1] - (int64_t)rel[p];
        const uint64_t *k = ki + rel[p], *v = vi + rel[p];
        sp_store_range(keys, first[p], n, key_bits, [&](int64_t i) { return k[i]; }, (int)threadIdx.x, (int)blockDim.x);
        sp_store_range(vals, first[p], n, val_bits, [&](int64_t i) { return v[i]; }, (int)threadIdx.x, (int)blockDim.x);
    }
}

// all seeds of one list back in the reference's (k-mer, value) form
__global__ void k_sp_dump_list(DevIndexView ix, uint32_t md, int64_t n_main, uint64_t *__restrict__ kmers,
                               uint64_t *__restrict__ vals) {
    const int64_t base = ix.md_off[md];
    const uint32_t *row = ix.part_tab + (int64_t)md * ix.P1;
    const uint64_t pfx = ix.masks[md >> 1] >> ((ix.K - ix.mask_prefix) << 1);
    const int P = ix.P1 - 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_main; i += (int64_t)gridDim.x * blockDim.x) {
        int lo = 0, hi = P; // partition of seed i: last row entry <= i
        while (lo + 1 < hi) {
            const int mid = (lo + hi) >> 1;
            if ((int64_t)row[mid] <= i)
                lo = mid;
            else
                hi = mid;
        }
        const uint64_t rem = lm_bits_get(ix.pk_keys, base + i, ix.key_bits);
        const uint64_t pv = lm_bits_get(ix.pk_vals, base + i, ix.gid_bits + ix.pos_bits + 1);
        kmers[i] = (((pfx << (ix.part_bases << 1)) | (uint64_t)lo) << ix.key_bits) | rem;
        vals[i] = lm_unpack_seed_val(pv, ix.g_bg[lm_packed_val_genome(pv, ix.pos_bits)], ix.pos_bits, (int)(md & 1));
    }
}

// The seeds [s0, s1) of the image - main seeds numbered as md_off counts them (FLAT = false) or outliers as out_off does
// (FLAT = true) - in the staging form SeedPacker::count / place consume: (mask, k-mer, value in the reference's layout) at
// i - s0.  [l0, l1) are the lists that hold them (sw_piece_lists).  The lanes run over the output seeds, so the packed reads
// and the three output streams of a wavefront are contiguous: 18 B written per seed, the bit fields read once.  A tile of
// blockDim.x seeds finds its first and last list and the partitions of its first and last seed once (uniform searches:
// scalar loads); a lane searches between those brackets only (lm_seed_walk.h), which is a handful of partitions wherever
// lists are longer than a tile.  The outlier lists are flat pairs: a copy with the mask id beside it.
// MODE says what genome key a value carries (lm_index_builder_add_index, lm_join_plan.h):
//   SP_DUMP_KEEP     the source's own key (new_bg unused): lm_index_builder_extend's base
//   SP_DUMP_REWRITE  new_bg[local record]; no entry of the table is JOIN_DROP.  Same access pattern, nothing else
//   SP_DUMP_COMPACT  new_bg[local record], and a seed whose record is JOIN_DROP is not written: every wavefront ballots
//                    "kept", its first lane reserves popcount slots of the output with ONE atomic on *n_out (zeroed by the
//                    host per piece) and the lanes write at that base + their rank among the kept lanes - a wavefront's
//                    three output streams stay contiguous, the order of the wavefronts in the output is whatever the
//                    atomics give (the packer's image does not depend on it).  At most s1 - s0 seeds are written.
// An outlier's value is in the reference's layout already: its record is found from the source's key through batch_first
// (sources are unsharded: lm_index_builder_add_index); a key outside the source's records (no index holds one) is dropped
// under COMPACT and never used as an index into the table.
enum { SP_DUMP_KEEP = 0, SP_DUMP_REWRITE = 1, SP_DUMP_COMPACT = 2 };
template <bool FLAT, int MODE>
__global__ __launch_bounds__(256) void k_sp_dump_range(DevIndexView ix, int64_t l0, int64_t l1, int64_t s0, int64_t s1,
                                                        uint16_t *__restrict__ s_mask, uint64_t *__restrict__ s_kmer,
                                                        uint64_t *__restrict__ s_val, const uint64_t *__restrict__ new_bg,
                                                        unsigned long long *__restrict__ n_out) {
    const int64_t *__restrict__ off = FLAT ? ix.out_off : ix.md_off;
    const int P = ix.P1 - 1;
    const int val_bits = ix.gid_bits + ix.pos_bits + 1;
    for (int64_t t0 = s0 + (int64_t)blockIdx.x * blockDim.x; t0 < s1; t0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t1 = (t0 + (int64_t)blockDim.x < s1 ? t0 + (int64_t)blockDim.x : s1) - 1;
        int64_t lf, ll;
        sw_tile_lists(off, l0, l1, t0, t1, &lf, &ll);
        int pf = 0, pl = P - 1;
        if (!FLAT) {
            pf = (int)sw_last_le(ix.part_tab + lf * ix.P1, 0, P - 1, t0 - off[lf]);
            pl = (int)sw_last_le(ix.part_tab + ll * ix.P1, lf == ll ? pf : 0, P - 1, t1 - off[ll]);
        }
        const int64_t i = t0 + threadIdx.x;
        if (MODE != SP_DUMP_COMPACT && i > t1) continue; // (COMPACT: every lane of the wavefront takes part in the ballot below)
        bool kept = i <= t1;
        int64_t md = 0;
        uint64_t kmer = 0, val = 0;
        if (kept) {
            md = sw_last_le(off, lf, ll, i);
            if (FLAT) {
                kmer = ix.out_kmers[i];
                val = ix.out_vals[i];
                if (MODE != SP_DUMP_KEEP) {
                    const uint64_t bg = val >> 30, batch = bg >> 17;
                    const int64_t local = batch < (uint64_t)ix.nbatches ? ix.batch_first[batch] + (int64_t)(bg & 0x1ffff) : -1;
                    if (local >= 0 && local < ix.ngenomes) {
                        const uint64_t nb = new_bg[local];
                        if (MODE == SP_DUMP_COMPACT && nb == ~0ull) kept = false;
                        val = (nb << 30) | (val & 0x3fffffffull);
                    } else if (MODE == SP_DUMP_COMPACT) {
                        kept = false;
                    }
                }
            } else {
                const int part = sw_partition(ix.part_tab + md * ix.P1, P, i - off[md], md == lf, pf, md == ll, pl);
                const uint64_t pfx = ix.masks[md >> 1] >> ((ix.K - ix.mask_prefix) << 1);
                const uint64_t rem = lm_bits_get(ix.pk_keys, i, ix.key_bits);
                const uint64_t pv = lm_bits_get(ix.pk_vals, i, val_bits);
                kmer = (((pfx << (ix.part_bases << 1)) | (uint64_t)part) << ix.key_bits) | rem;
                const uint64_t local = lm_packed_val_genome(pv, ix.pos_bits);
                uint64_t bg;
                if (MODE == SP_DUMP_KEEP) {
                    bg = ix.g_bg[local];
                } else { // (a value past the source's records - no image holds one - reads nothing outside the table)
                    bg = (int64_t)local < ix.ngenomes ? new_bg[local] : ~0ull;
                    if (MODE == SP_DUMP_COMPACT && bg == ~0ull) kept = false;
                }
                val = lm_unpack_seed_val(pv, bg, ix.pos_bits, (int)(md & 1));
            }
        }
        int64_t o = i - s0;
        if (MODE == SP_DUMP_COMPACT) {
            const unsigned long long bal = __ballot(kept);
            const int lane = (int)(threadIdx.x & 63u);
            unsigned long long base = 0;
            if (lane == 0 && bal) base = atomicAdd(n_out, (unsigned long long)__popcll(bal));
            base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            o = (int64_t)base + __popcll(bal & ((1ull << lane) - 1ull));
        }
        if (kept && (MODE != SP_DUMP_COMPACT || o < s1 - s0)) {
            s_mask[o] = (uint16_t)(md >> 1);
            s_kmer[o] = kmer;
            s_val[o] = val;
        }
    }
}

void sp_dump_range(const lm_index *src, hipStream_t st, const std::vector<int64_t> &off, bool flat, int64_t s0, int64_t s1,
                   uint16_t *s_mask, uint64_t *s_kmer, uint64_t *s_val, const uint64_t *new_bg, unsigned long long *n_out) {
    if (s1 <= s0) return;
    const int64_t nmd = (int64_t)off.size() - 1;
    if (s0 < 0 || s1 > off[(size_t)nmd]) throw HipError("seed image: a decode piece outside the image");
    if (n_out && !new_bg) throw HipError("seed image: a compacting decode needs a rewrite table");
    int64_t l0, l1;
    sw_piece_lists(off.data(), nmd, s0, s1, &l0, &l1);
    // (a bandwidth kernel: at most 8 workgroups per CU, the rest of the piece by grid stride)
    const unsigned grid = (unsigned)std::min<int64_t>((s1 - s0 + 255) / 256, 2048);
    const int mode = !new_bg ? SP_DUMP_KEEP : n_out ? SP_DUMP_COMPACT : SP_DUMP_REWRITE;
#define SP_DUMP_LAUNCH(F, M)                                                                                                        \
    hipLaunchKernelGGL((k_sp_dump_range<F, M>), dim3(grid), dim3(256), 0, st, src->view, l0, l1, s0, s1, s_mask, s_kmer, s_val, new_bg, n_out)
    if (flat) {
        if (mode == SP_DUMP_KEEP) SP_DUMP_LAUNCH(true, SP_DUMP_KEEP);
        else if (mode == SP_DUMP_REWRITE) SP_DUMP_LAUNCH(true, SP_DUMP_REWRITE);
        else SP_DUMP_LAUNCH(true, SP_DUMP_COMPACT);
    } else {
        if (mode == SP_DUMP_KEEP) SP_DUMP_LAUNCH(false, SP_DUMP_KEEP);
        else if (mode == SP_DUMP_REWRITE) SP_DUMP_LAUNCH(false, SP_DUMP_REWRITE);
        else SP_DUMP_LAUNCH(false, SP_DUMP_COMPACT);
    }
#undef SP_DUMP_LAUNCH
    HIPCHK(hipGetLastError());
}

static int sp_grid(int64_t n, int block = 256) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 262144) g = 262144;
    return (int)g;
}

static SpParams sp_params(const SeedPacker &sp) {
    const lm_index *ix = sp.ix;
    SpParams p;
    p.masks = ix->view.masks;
    p.K = ix->host.k;
    p.p = ix->host.mask_prefix;
    p.a = sp.a;
    p.P1 = sp.P1;
    p.key_bits = sp.key_bits;
    p.gid_bits = sp.gid_bits;
    p.pos_bits = sp.pos_bits;
    p.M = ix->host.M;
    p.batch_first = ix->view.batch_first;
    p.nbatches = ix->view.nbatches;
    p.shard_rank = ix->view.shard_rank;
    p.shard_count = ix->view.shard_count;
    p.g2local = ix->view.g2local;
    return p;
}

void SeedPacker::begin(lm_index *ix_, int64_t local_genomes, int64_t max_genome_len) {
    ix = ix_;
    const HostIndex &h = ix->host;
    if (h.M > 65535) throw HipError("seed image: more than 65535 masks are not supported (16-bit mask ids in the loader's staging records; include/lexicmap_hip.h)");
    a = std::min(h.anchor_prefix, 6);
    while (a > 0 && h.mask_prefix + a >= h.k) a--;
    P1 = (1 << (2 * a)) + 1;
    key_bits = 2 * (h.k - h.mask_prefix - a);
    gid_bits = bits_for(std::max<int64_t>(local_genomes, 2));
    pos_bits = bits_for(std::max<int64_t>(max_genome_len + 1, 2));
    if (pos_bits > 28) throw HipError("seed image: genome longer than 2^28 bases (lib-index-build.go:421-425)");
    if (gid_bits + pos_bits + 1 > 64) throw HipError("seed image: value does not fit 64 bits");
    const int64_t nmd = 2ll * h.M;
    ix->d_part_tab.alloc_exact((size_t)(nmd * P1), true, ix->lane[0].main.st);
    out_cnt.alloc_exact((size_t)nmd + 1, true, ix->lane[0].main.st);
    n_main = n_out = 0;
    placing = false;
}

void SeedPacker::count(const uint16_t *mask, const uint64_t *kmer, const uint64_t *val, int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_sp_count, dim3(sp_grid(n)), dim3(256), 0, ix->lane[0].main.st, sp_params(*this), mask, kmer, val, n,
                       ix->d_part_tab.p, out_cnt.p);
}

void SeedPacker::end_count() {
    const hipStream_t st = ix->lane[0].main.st;
    const int64_t nmd = 2ll * ix->host.M;
    DBuf<unsigned long long> md_cnt;
    md_cnt.alloc_exact((size_t)nmd + 1, true, st);
    hipLaunchKernelGGL(k_sp_scan_rows, dim3((unsigned)std::min<int64_t>(nmd, 65536)), dim3(256), 0, st, ix->d_part_tab.p,
                       P1, nmd, md_cnt.p);
    ix->d_md_off.alloc_exact((size_t)nmd + 1);
    ix->d_out_off.alloc_exact((size_t)nmd + 1);
    prim_scan_to_i64(st, ix->lane[0].main.tmp, md_cnt.p, (size_t)nmd, ix->d_md_off.p);
    prim_scan_to_i64(st, ix->lane[0].main.tmp, out_cnt.p, (size_t)nmd, ix->d_out_off.p);
    int64_t tot[2];
    HIPCHK(hipMemcpyAsync(&tot[0], ix->d_md_off.p + nmd, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&tot[1], ix->d_out_off.p + nmd, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    n_main = tot[0];
    n_out = tot[1];
    const int val_bits = gid_bits + pos_bits + 1;
    // +2 words: lm_bits_get may touch the word after the last element
    ix->d_pk_keys.alloc_exact((size_t)((n_main * key_bits + 63) / 64 + 2), true, st);
    ix->d_pk_vals.alloc_exact((size_t)((n_main * val_bits + 63) / 64 + 2), true, st);
    ix->d_out_kmers.alloc_exact((size_t)n_out + 1);
    ix->d_out_vals.alloc_exact((size_t)n_out + 1);
    HIPCHK(hipMemsetAsync(out_cnt.p, 0, ((size_t)nmd + 1) * sizeof(unsigned long long), st)); // now the outlier cursors
    placing = true;
}

void SeedPacker::place(const uint16_t *mask, const uint64_t *kmer, const uint64_t *val, int64_t n) {
    if (n <= 0) return;
    if (!placing) throw HipError("SeedPacker::place before end_count");
    hipLaunchKernelGGL(k_sp_place, dim3(sp_grid(n)), dim3(256), 0, ix->lane[0].main.st, sp_params(*this), mask, kmer, val, n,
                       ix->d_part_tab.p, ix->d_md_off.p, ix->d_pk_keys.p, ix->d_pk_vals.p, ix->d_out_off.p, out_cnt.p,
                       ix->d_out_kmers.p, ix->d_out_vals.p);
}

void SeedPacker::finish() {
    const hipStream_t st = ix->lane[0].main.st;
    const HostIndex &h = ix->host;
    const int64_t nmd = 2ll * h.M;
    const int val_bits = gid_bits + pos_bits + 1;
    // ---- main partitions
    // (a partition counts as big above SP_MAXN seeds, so there are fewer than n_main / SP_MAXN of them: 6e5 at C3, 1.5e6 in a
    // 250 000-genome shard of C4)
    const unsigned long long big_cap = (unsigned long long)(n_main / SP_MAXN) + 1024;
    DBuf<unsigned long long> big, nbig;
    big.alloc_exact(big_cap);
    nbig.alloc_exact(1, true, st);
    if (n_main > 0) {
        const int64_t nparts = nmd * (P1 - 1);
        const int dbg_mode = 0; // (the kernel's timing-experiment modes are not reachable any more)
        const double t0 = now_ms();
        hipLaunchKernelGGL(k_sp_sort_parts, dim3((unsigned)std::min<int64_t>(nparts, (int64_t)1 << 22)), dim3(64), 0, st,
                           ix->d_part_tab.p, ix->d_md_off.p, P1, nmd, key_bits, val_bits, ix->d_pk_keys.p, ix->d_pk_vals.p,
                           big.p, big_cap, nbig.p, dbg_mode);
        unsigned long long nb = 0;
        HIPCHK(hipMemcpyAsync(&nb, nbig.p, sizeof nb, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (getenv("LM_DEBUG"))
            fprintf(stderr, "[lm] seed image: partition sort kernel %.0f ms (mode %d), %llu partitions above %d seeds\n", now_ms() - t0,
                    dbg_mode, nb, SP_MAXN);
        if (nb > big_cap) throw HipError("seed image: too many partitions above the LDS sorter's size");
        if (nb > 0) {
            const double t1 = now_ms();
            DBuf<int64_t> bfirst, bcnt, boff;
            bfirst.alloc_exact((size_t)nb + 1);
            bcnt.alloc_exact((size_t)nb + 1, true, st);
            boff.alloc_exact((size_t)nb + 2);
            hipLaunchKernelGGL(k_sp_big_info, dim3(sp_grid((int64_t)nb)), dim3(256), 0, st, big.p, (int64_t)nb, ix->d_part_tab.p,
                               ix->d_md_off.p, P1, bfirst.p, bcnt.p);
            prim_scan_to_i64(st, ix->lane[0].main.tmp, bcnt.p, (size_t)nb, boff.p);
            std::vector<int64_t> off((size_t)nb + 1);
            HIPCHK(hipMemcpyAsync(off.data(), boff.p, ((size_t)nb + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            // batches of whole partitions: 4 temporary u64 arrays, at most a quarter of what is free and 2^31 elements
            size_t fr = 0, tot = 0;
            (void)hipMemGetInfo(&fr, &tot);
            int64_t batch = std::min<int64_t>(((int64_t)1 << 31) - 1, std::max<int64_t>((int64_t)(fr / 4 / 40), 1 << 20));
            DBuf<uint64_t> k0, k1, v0, v1;
            DBuf<uint32_t> rel;
            int64_t done_elems = 0;
            for (size_t b0 = 0; b0 < (size_t)nb;) {
                size_t b1 = b0 + 1;
                while (b1 < (size_t)nb && off[b1 + 1] - off[b0] <= batch) b1++;
                const int64_t E = off[b1] - off[b0], nseg = (int64_t)(b1 - b0);
                if (E >= (int64_t)1 << 32) throw HipError("seed image: one partition holds more than 2^32 seeds");
                k0.ensure((size_t)E);
                k1.ensure((size_t)E);
                v0.ensure((size_t)E);
                v1.ensure((size_t)E);
                rel.ensure((size_t)nseg + 1);
                hipLaunchKernelGGL(k_sp_unpack_many, dim3(sp_grid(E)), dim3(256), 0, st, ix->d_pk_keys.p, ix->d_pk_vals.p, key_bits,
                                   val_bits, bfirst.p + b0, boff.p + b0, nseg, off[b0], E, k0.p, v0.p);
                hipLaunchKernelGGL(k_sp_rel_offsets, dim3(sp_grid(nseg + 1)), dim3(256), 0, st, boff.p + b0, nseg, off[b0], rel.p);
                prim_segmented_sort_pairs(st, ix->lane[0].main.tmp, k0.p, k1.p, v0.p, v1.p, (size_t)E, (size_t)nseg, rel.p, 0, key_bits);
                hipLaunchKernelGGL(k_sp_repack_many, dim3((unsigned)std::min<int64_t>(nseg, 65536)), dim3(256), 0, st,
                                   ix->d_pk_keys.p, ix->d_pk_vals.p, key_bits, val_bits, bfirst.p + b0, rel.p, nseg, k1.p, v1.p);
                HIPCHK(hipStreamSynchronize(st));
                done_elems += E;
                b0 = b1;
            }
            if (getenv("LM_DEBUG"))
                fprintf(stderr, "[lm] seed image: %llu large partitions (%lld seeds) sorted by rocPRIM in %.0f ms\n", nb,
                        (long long)done_elems, now_ms() - t1);
        }
    }
    // ---- outlier lists: per list by k-mer
    if (n_out > 0) {
        DBuf<uint64_t> k1, v1;
        k1.alloc_exact((size_t)n_out + 1);
        v1.alloc_exact((size_t)n_out + 1);
        prim_segmented_sort_pairs(st, ix->lane[0].main.tmp, ix->d_out_kmers.p, k1.p, ix->d_out_vals.p, v1.p, (size_t)n_out, (size_t)nmd,
                                  ix->d_out_off.p, 0, 2 * h.k);
        HIPCHK(hipStreamSynchronize(st));
        std::swap(ix->d_out_kmers.p, k1.p);
        std::swap(ix->d_out_kmers.cap, k1.cap);
        std::swap(ix->d_out_vals.p, v1.p);
        std::swap(ix->d_out_vals.cap, v1.cap);
    }
    HIPCHK(hipStreamSynchronize(st));
    out_cnt.release();
    DevIndexView &v = ix->view;
    v.part_bases = a;
    v.P1 = P1;
    v.key_bits = key_bits;
    v.gid_bits = gid_bits;
    v.pos_bits = pos_bits;
    v.pk_keys = ix->d_pk_keys.p;
    v.pk_vals = ix->d_pk_vals.p;
    v.part_tab = ix->d_part_tab.p;
    v.md_off = ix->d_md_off.p;
    v.out_kmers = ix->d_out_kmers.p;
    v.out_vals = ix->d_out_vals.p;
    v.out_off = ix->d_out_off.p;
    ix->n_seeds = n_main + n_out;
    ix->n_seeds_outlier = n_out;
    ix->seed_bytes = (int64_t)(ix->d_pk_keys.cap * 8 + ix->d_pk_vals.cap * 8 + ix->d_part_tab.cap * 4 + ix->d_md_off.cap * 8 +
                               ix->d_out_off.cap * 8 + ix->d_out_kmers.cap * 8 + ix->d_out_vals.cap * 8);
}

} // namespace lm

// (k-mer, value) pairs stored under one mask, both directions, in the reference's in-memory form: what `lexicmap utils
// kmers -m <mask>` lists (cmd/kmers.go:101-180) and what kv.Reader.ReadDataOfAMaskAsList returns (kv-reader.go:762).
// Inspection / test entry point: the search path never unpacks lists.
extern "C" lm_status lm_index_mask_seeds(lm_index *ix, int32_t mask, uint64_t *kmers, uint64_t *vals, size_t cap, size_t *n_out) {
    if (!ix || mask < 0 || mask >= ix->host.M || !n_out) return LM_ERR_ARG;
    try {
        std::lock_guard<std::mutex> lock(ix->mu);
        HIPCHK(hipSetDevice(ix->device));
        const int64_t nmd = 2ll * ix->host.M;
        int64_t mdo[3], oo[3];
        HIPCHK(hipMemcpy(mdo, ix->d_md_off.p + 2 * mask, sizeof mdo, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(oo, ix->d_out_off.p + 2 * mask, sizeof oo, hipMemcpyDeviceToHost));
        (void)nmd;
        const size_t total = (size_t)(mdo[2] - mdo[0]) + (size_t)(oo[2] - oo[0]);
        *n_out = total;
        if (cap == 0 || (!kmers && !vals)) return LM_OK; // size query
        if (!kmers || !vals || cap < total) {
            ix->err = "lm_index_mask_seeds: buffer too small (cap < *n) or a NULL array";
            return LM_ERR_ARG; // nothing was written; *n holds the count to allocate
        }
        DBuf<uint64_t> dk, dv;
        size_t w = 0;
        for (int dir = 0; dir < 2; dir++) {
            const int64_t nm = mdo[dir + 1] - mdo[dir], no = oo[dir + 1] - oo[dir];
            if (nm > 0) {
                dk.ensure((size_t)nm);
                dv.ensure((size_t)nm);
                hipLaunchKernelGGL(lm::k_sp_dump_list, dim3(lm::sp_grid(nm)), dim3(256), 0, ix->lane[0].main.st, ix->view,
                                   (uint32_t)(2 * mask + dir), nm, dk.p, dv.p);
                HIPCHK(hipMemcpyAsync(kmers + w, dk.p, (size_t)nm * 8, hipMemcpyDeviceToHost, ix->lane[0].main.st));
                HIPCHK(hipMemcpyAsync(vals + w, dv.p, (size_t)nm * 8, hipMemcpyDeviceToHost, ix->lane[0].main.st));
                HIPCHK(hipStreamSynchronize(ix->lane[0].main.st));
                w += (size_t)nm;
            }
            if (no > 0) {
                HIPCHK(hipMemcpy(kmers + w, ix->d_out_kmers.p + oo[dir], (size_t)no * 8, hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(vals + w, ix->d_out_vals.p + oo[dir], (size_t)no * 8, hipMemcpyDeviceToHost));
                w += (size_t)no;
            }
        }
        return LM_OK;
    } catch (const std::exception &e) {
        ix->err = e.what();
        return LM_ERR_HIP;
    }
}

// ---- seed positions and seed distances of genome records --------------------------------------------------
// lm_index_seed_positions / lm_index_seed_distances: the forward seeds of the selected records leave the image as
// slot << 32 | loc (k_sp_seed_locs), one 64-bit radix sort puts them in selection and position order, k_sp_seed_segment
// cuts them into the per-record lists, k_sd_pass applies the distance rule of lm_seed_dist.h.
namespace lm {

// which records are wanted: main seeds carry a local record number, outliers the record's key
struct SeedSelDev {
    const int32_t *slot_of_local; // [nlocal] slot in the selection, -1: not selected
    int64_t nlocal;
    const uint64_t *okeys;        // [nsel] the selected keys ascending
    const int32_t *oslot;         // [nsel] their slots
    int32_t nsel;
};

__device__ __forceinline__ int sp_lane_rank(unsigned long long bal) { // kept lanes below this one (mbcnt)
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// The forward seeds [s0, s1) - numbered by `foff` ([M + 1]: the even lists md = 2 m of md_off back to back; FLAT: of out_off)
// - of the masks [l0, l1) that hold them, as slot << 32 | loc for the seeds of selected records.  A bandwidth kernel
// beside k_sp_dump_range: the lanes run over the seeds, a tile of blockDim.x seeds brackets its masks once
// (lm_seed_walk.h), only the packed VALUES are read (the partition of a seed does not matter here).  Every wavefront
// ballots "kept", its first lane reserves popcount slots with one vector atomic on *n_out, the lanes write at that base +
// their rank; a store is guarded by `cap`.  COUNT: the atomics only (the size of the key array of a partial selection).
template <bool FLAT, bool COUNT>
__global__ __launch_bounds__(256) void k_sp_seed_locs(DevIndexView ix, const int64_t *__restrict__ foff, int64_t l0, int64_t l1,
                                                       int64_t s0, int64_t s1, SeedSelDev sel, uint64_t *__restrict__ out,
                                                       unsigned long long cap, unsigned long long *__restrict__ n_out) {
    const int64_t *__restrict__ off = FLAT ? ix.out_off : ix.md_off;
    const int val_bits = ix.gid_bits + ix.pos_bits + 1;
    const uint64_t loc_mask = (1ull << (ix.pos_bits + 1)) - 1ull;
    const int lane = (int)(threadIdx.x & 63u);
    for (int64_t t0 = s0 + (int64_t)blockIdx.x * blockDim.x; t0 < s1; t0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t1 = (t0 + (int64_t)blockDim.x < s1 ? t0 + (int64_t)blockDim.x : s1) - 1;
        int64_t lf, ll;
        sw_tile_lists(foff, l0, l1, t0, t1, &lf, &ll);
        const int64_t i = t0 + threadIdx.x;
        int32_t slot = -1;
        uint32_t loc = 0;
        if (i <= t1) {
            const int64_t m = sw_last_le(foff, lf, ll, i);
            const int64_t src = off[2 * m] + (i - foff[m]);
            if (FLAT) {
                const uint64_t val = ix.out_vals[src], bg = val >> 30;
                if (!(val & 1ull) && sel.nsel > 0) {
                    const int64_t j = sw_last_le(sel.okeys, 0, (int64_t)sel.nsel - 1, (int64_t)bg);
                    if (sel.okeys[j] == bg) slot = sel.oslot[j];
                }
                loc = (uint32_t)(val >> 1) & 0x1fffffffu;
            } else {
                const uint64_t pv = lm_bits_get(ix.pk_vals, src, val_bits);
                const uint64_t local = lm_packed_val_genome(pv, ix.pos_bits);
                if ((int64_t)local < sel.nlocal) slot = sel.slot_of_local[local];
                loc = (uint32_t)(pv & loc_mask);
            }
        }
        const bool kept = slot >= 0;
        const unsigned long long bal = __ballot(kept);
        unsigned long long base = 0;
        if (lane == 0 && bal) base = atomicAdd(n_out, (unsigned long long)__popcll(bal));
        if (!COUNT) {
            base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) |
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            const unsigned long long o = base + (unsigned long long)sp_lane_rank(bal);
            if (kept && o < cap) out[o] = ((uint64_t)(uint32_t)slot << 32) | loc;
        }
    }
}

// sorted entries -> off[nsel + 1] (first entry of every slot; a slot without entries starts where the next one does) and locs
__global__ __launch_bounds__(256) void k_sp_seed_segment(const uint64_t *__restrict__ ent, int64_t n, int32_t nsel,
                                                          int64_t *__restrict__ off, uint32_t *__restrict__ locs) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e <= n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t hi = e < n ? (int64_t)(ent[e] >> 32) : (int64_t)nsel;
        const int64_t lo = e > 0 ? (int64_t)(ent[e - 1] >> 32) + 1 : 0;
        for (int64_t s = lo; s <= hi && s <= (int64_t)nsel; s++) off[s] = e;
        if (e < n) locs[e] = (uint32_t)ent[e];
    }
}

struct SdArgs {
    const uint64_t *ent; // sorted slot << 32 | loc
    int64_t n, ntiles;
    const int32_t *coff;    // [nsel + 1] CSR of the contig starts of the selected records
    const uint32_t *cstart;
    uint32_t min_dist, hist_bins, hist_width;
    unsigned long long *rec_max; // [nsel] dist << 32 | ~pos: the largest dist, the smallest position among equals
    uint32_t *rec_seeded;        // [nsel] contigs with a seed
    unsigned long long *hist;    // [hist_bins]
    uint32_t *tile_cnt;          // [ntiles + 1] reported positions per tile of 256 entries (EMIT = false writes it)
    const int64_t *tile_off;     // its exclusive scan (EMIT = true reads it)
    lm_seed_dist_row *rows;
};

// One lane per sorted entry, tiles of 256 entries.  EMIT = false: per record the largest distance (reduced over the lanes
// of a wavefront that share a record, one atomic per wavefront and record), the seeded contigs, the histogram of the
// reported distances in LDS (flushed once per workgroup) and the number of reported entries of every tile.  EMIT = true,
// after a scan of those numbers: the reported rows at tile offset + wavefront offset + rank among the reporting lanes -
// the order of the sorted entries, not the arrival order of an atomic.
template <bool EMIT> __global__ __launch_bounds__(256) void k_sd_pass(SdArgs a) {
    extern __shared__ uint32_t sd_lds[]; // [hist_bins] (EMIT = false)
    __shared__ uint32_t wcnt[4];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    if (!EMIT) {
        for (uint32_t b = threadIdx.x; b < a.hist_bins; b += blockDim.x) sd_lds[b] = 0;
        __syncthreads();
    }
    for (int64_t ti = blockIdx.x; ti < a.ntiles; ti += gridDim.x) {
        const int64_t e = ti * 256 + threadIdx.x;
        const bool act = e < a.n;
        uint32_t slot = 0, loc = 0;
        SdEntry en = {0, 0, 0, false};
        if (act) {
            const uint64_t k = a.ent[e];
            slot = (uint32_t)(k >> 32);
            loc = (uint32_t)k;
            uint64_t kp = 0;
            if (e > 0) kp = a.ent[e - 1];
            const int32_t c0 = a.coff[slot];
            en = sd_entry(a.cstart + c0, a.coff[slot + 1] - c0, loc >> 1, e > 0 && (uint32_t)(kp >> 32) == slot, (uint32_t)kp >> 1);
        }
        const bool rep = act && sd_reported(en.dist, a.min_dist);
        const unsigned long long bal = __ballot(rep);
        if (lane == 0) wcnt[w] = (uint32_t)__popcll(bal);
        __syncthreads();
        if (!EMIT) {
            if (threadIdx.x == 0) a.tile_cnt[ti] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            if (rep && a.hist_bins) atomicAdd(&sd_lds[sd_bin(en.dist, a.hist_bins, a.hist_width)], 1u);
            if (act && en.first) atomicAdd(&a.rec_seeded[slot], 1u);
            // the largest distance: the entries are sorted, so a wavefront holds a few records at most
            const unsigned long long v = act ? ((unsigned long long)en.dist << 32) | (0xffffffffu - (loc >> 1)) : 0ull;
            unsigned long long todo = __ballot(act);
            while (todo) {
                const int first = __ffsll((long long)todo) - 1;
                const uint32_t s = (uint32_t)__shfl((int)slot, first);
                const bool mine = act && slot == s;
                uint32_t hi = mine ? (uint32_t)(v >> 32) : 0u, lo = mine ? (uint32_t)v : 0u;
                for (int d = 32; d > 0; d >>= 1) {
                    const uint32_t ohi = (uint32_t)__shfl_xor((int)hi, d), olo = (uint32_t)__shfl_xor((int)lo, d);
                    if (ohi > hi || (ohi == hi && olo > lo)) {
                        hi = ohi;
                        lo = olo;
                    }
                }
                if (lane == first) atomicMax(&a.rec_max[s], ((unsigned long long)hi << 32) | lo);
                todo &= ~__ballot(mine);
            }
        } else if (rep) {
            int64_t o = a.tile_off[ti] + sp_lane_rank(bal);
            for (int x = 0; x < w; x++) o += wcnt[x];
            lm_seed_dist_row r;
            r.record = slot;
            r.contig = (uint32_t)en.contig;
            r.pos = loc >> 1;
            r.pos_in_contig = (loc >> 1) - en.start;
            r.strand = loc & 1u;
            r.dist = en.dist;
            a.rows[o] = r;
        }
        __syncthreads(); // (wcnt is written again by the next tile)
    }
    if (!EMIT) {
        __syncthreads();
        for (uint32_t b = threadIdx.x; b < a.hist_bins; b += blockDim.x)
            if (sd_lds[b]) atomicAdd(&a.hist[b], (unsigned long long)sd_lds[b]);
    }
}

__global__ void k_sd_records(const uint64_t *__restrict__ keys, const int64_t *__restrict__ off, const int32_t *__restrict__ coff,
                             const unsigned long long *__restrict__ rec_max, const uint32_t *__restrict__ rec_seeded, int32_t nsel,
                             lm_seed_dist_rec *__restrict__ recs) {
    for (int32_t s = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x); s < nsel; s += (int32_t)(gridDim.x * blockDim.x)) {
        lm_seed_dist_rec r;
        r.key = keys[s];
        r.seeds = off[s + 1] - off[s];
        r.max_dist = (uint32_t)(rec_max[s] >> 32);
        r.max_dist_pos = r.seeds > 0 ? 0xffffffffu - (uint32_t)rec_max[s] : 0u;
        r.contigs = coff[s + 1] - coff[s];
        r.contigs_without_seeds = r.contigs - (int32_t)rec_seeded[s];
        recs[s] = r;
    }
}

// the selected records' sorted entries, position lists and tables on the device
struct SeedLists {
    std::vector<uint64_t> keys;     // [nsel] record keys in selection order
    std::vector<int64_t> local;     // [nsel] their local record numbers
    DBuf<uint64_t> ent, ent2;       // ent: the sorted entries
    DBuf<int64_t> off;              // [nsel + 1]
    DBuf<uint32_t> locs;            // [n]
    int64_t n = 0;
};

template <typename T> static void sp_upload(lm_index *ix, DBuf<T> &d, const std::vector<T> &v) {
    d.alloc_exact(std::max<size_t>(v.size(), 1));
    if (!v.empty()) HIPCHK(hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, ix->lane[0].main.st));
}

static void seed_lists(lm_index *ix, const char *who, const uint64_t *keys, size_t nkeys, SeedLists &L) {
    const hipStream_t st = ix->lane[0].main.st;
    const HostIndex &h = ix->host;
    const int64_t nlocal = (int64_t)h.genomes.size();
    const int M = h.M;
    const bool dbg = getenv("LM_DEBUG") != nullptr;
    if (!keys && nkeys > 0) throw ArgError(std::string(who) + ": keys is NULL but nkeys is not 0");
    if (nkeys >= ((size_t)1 << 31)) throw ArgError(std::string(who) + ": more than 2^31 keys");
    // ---- the selection
    const bool all = keys == nullptr;
    std::vector<int32_t> slot_of_local((size_t)nlocal, -1);
    if (all) {
        for (int64_t l = 0; l < nlocal; l++) {
            L.keys.push_back(h.genomes[(size_t)l].bg);
            L.local.push_back(l);
            slot_of_local[(size_t)l] = (int32_t)l;
        }
    } else {
        const auto &local_of = ix->bg2local; // key -> local record, kept by the handle (lm_index_set_genome_filter uses it too)
        for (size_t s = 0; s < nkeys; s++) {
            const auto it = local_of.find(keys[s]);
            const std::string name = "key " + std::to_string(keys[s]) + " (batch " + std::to_string(keys[s] >> 17) + ", index " + std::to_string(keys[s] & 0x1ffff) + ")";
            if (it == local_of.end()) {
                if (h.other_of.count(keys[s]))
                    throw ArgError(std::string(who) + ": " + name + " is a record of another shard (this handle is shard " + std::to_string(h.shard_rank) +
                                  " of " + std::to_string(h.shard_count) + " and answers for its own records)");
                throw ArgError(std::string(who) + ": " + name + " is no record of this index");
            }
            if (slot_of_local[(size_t)it->second] >= 0) throw ArgError(std::string(who) + ": " + name + " is given twice");
            slot_of_local[(size_t)it->second] = (int32_t)s;
            L.keys.push_back(keys[s]);
            L.local.push_back((int64_t)it->second);
        }
    }
    const int32_t nsel = (int32_t)L.keys.size();
    std::vector<std::pair<uint64_t, int32_t>> sorted_keys;
    for (int32_t s = 0; s < nsel; s++) sorted_keys.emplace_back(L.keys[(size_t)s], s);
    std::sort(sorted_keys.begin(), sorted_keys.end());
    std::vector<uint64_t> okeys;
    std::vector<int32_t> oslot;
    for (auto &e : sorted_keys) {
        okeys.push_back(e.first);
        oslot.push_back(e.second);
    }
    // ---- the forward lists numbered back to back
    std::vector<int64_t> md_off((size_t)2 * M + 1), out_off((size_t)2 * M + 1), foff[2];
    HIPCHK(hipMemcpyAsync(md_off.data(), ix->d_md_off.p, md_off.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_off.data(), ix->d_out_off.p, out_off.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int f = 0; f < 2; f++) {
        const std::vector<int64_t> &o = f ? out_off : md_off;
        foff[f].assign((size_t)M + 1, 0);
        for (int m = 0; m < M; m++) foff[f][(size_t)m + 1] = foff[f][(size_t)m] + (o[(size_t)2 * m + 1] - o[(size_t)2 * m]);
    }
    const int64_t nfwd[2] = {foff[0].back(), foff[1].back()};
    DBuf<int32_t> d_slot, d_oslot;
    DBuf<uint64_t> d_okeys;
    DBuf<int64_t> d_foff[2];
    DBuf<unsigned long long> d_cnt;
    sp_upload(ix, d_slot, slot_of_local);
    sp_upload(ix, d_okeys, okeys);
    sp_upload(ix, d_oslot, oslot);
    sp_upload(ix, d_foff[0], foff[0]);
    sp_upload(ix, d_foff[1], foff[1]);
    d_cnt.alloc_exact(1, true, st);
    const SeedSelDev sel{d_slot.p, nlocal, d_okeys.p, d_oslot.p, nsel};
    // pieces: at most 2^26 seeds per launch as for lm_index_builder_extend; tests make them small (no result depends on it)
    int64_t piece = (int64_t)1 << 26;
    if (const char *e = getenv("LM_SEEDPOS_PIECE_SEEDS")) piece = std::max<int64_t>(4, atoll(e));
    int npieces = 0;
    auto walk = [&](bool count, uint64_t *out, unsigned long long cap) {
        for (int f = 0; f < 2; f++)
            for (int64_t s0 = 0; s0 < nfwd[f]; s0 += piece) {
                const int64_t s1 = std::min(nfwd[f], s0 + piece);
                int64_t l0, l1;
                sw_piece_lists(foff[f].data(), M, s0, s1, &l0, &l1);
                const unsigned grid = (unsigned)std::min<int64_t>((s1 - s0 + 255) / 256, 2048); // at most 8 workgroups per CU, then a grid stride
#define SP_LOCS_LAUNCH(F, C) hipLaunchKernelGGL((k_sp_seed_locs<F, C>), dim3(grid), dim3(256), 0, st, ix->view, d_foff[f].p, l0, l1, s0, s1, sel, out, cap, d_cnt.p)
                if (f) {
                    if (count) SP_LOCS_LAUNCH(true, true);
                    else SP_LOCS_LAUNCH(true, false);
                } else {
                    if (count) SP_LOCS_LAUNCH(false, true);
                    else SP_LOCS_LAUNCH(false, false);
                }
#undef SP_LOCS_LAUNCH
                npieces++;
            }
        HIPCHK(hipGetLastError());
        unsigned long long c = 0;
        HIPCHK(hipMemcpyAsync(&c, d_cnt.p, sizeof c, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        return (int64_t)c;
    };
    // ---- the size of the key array: every forward seed when every record is wanted, else a counting pass
    const double t0 = now_ms();
    int64_t n = nsel > 0 ? nfwd[0] + nfwd[1] : 0; // (keys given, nkeys = 0: no record, no seed, nothing is walked)
    if (!all && nsel > 0) {
        n = walk(true, nullptr, 0);
        HIPCHK(hipMemsetAsync(d_cnt.p, 0, sizeof(unsigned long long), st));
    }
    const double t1 = now_ms();
    try {
        L.ent.alloc_exact((size_t)n + 1);
        L.ent2.alloc_exact((size_t)n + 1);
        L.off.alloc_exact((size_t)nsel + 1);
        L.locs.alloc_exact((size_t)n + 1);
    } catch (const DeviceOOM &e) {
        throw DeviceOOM(std::string(who) + ": the " + std::to_string(n) + " forward seeds of the selection need 2 x 8 B of sort keys and 4 B of "
                        "position list each (" + std::to_string((n * 20) >> 20) + " MB) on the device beside the index: " + e.what());
    }
    npieces = 0;
    const double t1b = now_ms(); // (the allocations are not the extract kernel's time)
    const int64_t got = nsel > 0 ? walk(false, L.ent2.p, (unsigned long long)n) : 0;
    if (got != n) throw HipError(std::string(who) + ": the image holds " + std::to_string(got) + " forward seeds of the selection where " + std::to_string(n) + " were counted");
    const double t2 = now_ms();
    try {
        prim_sort_keys(st, ix->lane[0].main.tmp, L.ent2.p, L.ent.p, (size_t)n, 0, 32 + bits_for(std::max<int64_t>(nsel, 2)));
    } catch (const DeviceOOM &e) {
        throw DeviceOOM(std::string(who) + ": the radix sort of " + std::to_string(n) + " keys needs scratch beside its two key arrays: " + e.what());
    }
    if (dbg) HIPCHK(hipStreamSynchronize(st));
    const double t3 = now_ms();
    hipLaunchKernelGGL(k_sp_seed_segment, dim3(sp_grid(n + 1)), dim3(256), 0, st, L.ent.p, n, nsel, L.off.p, L.locs.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    L.ent2.release(); // (the unsorted keys: the distance pass allocates its rows in their place)
    L.n = n;
    if (dbg) {
        const double rd = (double)nfwd[0] * (ix->view.gid_bits + ix->view.pos_bits + 1) / 8.0 + (double)nfwd[1] * 8.0;
        fprintf(stderr, "[lm] seed positions: %d records, %lld of %lld + %lld forward seeds (main + outlier): count %.3f ms, allocations %.3f ms, "
                        "extract %.3f ms (%d pieces of %lld, %.0f bytes of values read, %.1f GB/s), sort %.3f ms, segment %.3f ms\n",
                (int)nsel, (long long)n, (long long)nfwd[0], (long long)nfwd[1], t1 - t0, t1b - t1, t2 - t1b, npieces, (long long)piece, rd,
                rd / std::max(1e-6, t2 - t1b) / 1e6, t3 - t2, now_ms() - t3);
    }
}

} // namespace lm

struct lm_seedpos {
    std::vector<uint64_t> keys;
    std::vector<int64_t> off;
    std::vector<uint32_t> locs;
};
struct lm_seed_dist {
    std::vector<lm_seed_dist_rec> recs;
    std::vector<uint64_t> hist;
    std::vector<lm_seed_dist_row> rows;
};

static const char *const SEED_NOMEM = "seed positions: the host could not hold the result"; // (both calls: lm::guarded)

extern "C" lm_status lm_index_seed_positions(lm_index *ix, const uint64_t *keys, size_t nkeys, lm_seedpos **out) {
    if (!ix || !out) return LM_ERR_ARG;
    *out = nullptr;
    std::unique_ptr<lm_seedpos> res(new lm_seedpos());
    const hipStream_t stream = ix->lane[0].main.st;
    const lm_status st = guarded(ix, SEED_NOMEM, [&]() {
        lm::SeedLists L;
        lm::seed_lists(ix, "lm_index_seed_positions", keys, nkeys, L);
        res->keys = L.keys;
        res->off.resize(L.keys.size() + 1);
        res->locs.resize((size_t)L.n);
        HIPCHK(hipMemcpyAsync(res->off.data(), L.off.p, res->off.size() * 8, hipMemcpyDeviceToHost, stream));
        if (L.n > 0) HIPCHK(hipMemcpyAsync(res->locs.data(), L.locs.p, (size_t)L.n * 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    });
    if (st == LM_OK) *out = res.release();
    return st;
}
extern "C" size_t lm_seedpos_get(const lm_seedpos *sp, const uint64_t **keys, const int64_t **off, const uint32_t **locs) {
    if (!sp) return 0;
    if (keys) *keys = sp->keys.data();
    if (off) *off = sp->off.data();
    if (locs) *locs = sp->locs.data();
    return sp->keys.size();
}
extern "C" void lm_seedpos_free(lm_seedpos *sp) { delete sp; }

extern "C" lm_status lm_index_seed_distances(lm_index *ix, const uint64_t *keys, size_t nkeys, const lm_seed_dist_opt *opt_in, lm_seed_dist **out) {
    using namespace lm;
    if (!ix || !out) return LM_ERR_ARG;
    *out = nullptr;
    lm_seed_dist_opt opt = {0, 0, 0, 0};
    if (opt_in) opt = *opt_in;
    std::unique_ptr<lm_seed_dist> res(new lm_seed_dist());
    const hipStream_t stream = ix->lane[0].main.st;
    const lm_status st = guarded(ix, SEED_NOMEM, [&]() {
        if (opt.hist_bins > 0 && opt.hist_width < 1) throw ArgError("lm_index_seed_distances: hist_bins = " + std::to_string(opt.hist_bins) + " with hist_width < 1");
        if (opt.hist_bins > 4096) throw ArgError("lm_index_seed_distances: hist_bins = " + std::to_string(opt.hist_bins) + " (at most 4096 counters)");
        SeedLists L;
        seed_lists(ix, "lm_index_seed_distances", keys, nkeys, L);
        const HostIndex &h = ix->host;
        const int32_t nsel = (int32_t)L.keys.size();
        // ---- the contig starts of the selected records as a CSR
        std::vector<int32_t> coff((size_t)nsel + 1, 0);
        std::vector<uint32_t> cstart;
        for (int32_t s = 0; s < nsel; s++) {
            const HostGenome &G = h.genomes[(size_t)L.local[(size_t)s]];
            const int32_t nc = std::max<int32_t>(1, (int32_t)G.seq_sizes.size());
            const size_t at = cstart.size();
            cstart.resize(at + (size_t)nc, 0u);
            if (!G.seq_sizes.empty()) sd_contig_starts(G.seq_sizes.data(), nc, h.contig_interval, cstart.data() + at);
            coff[(size_t)s + 1] = (int32_t)cstart.size();
        }
        const int64_t n = L.n, ntiles = (n + 255) / 256;
        DBuf<int32_t> d_coff;
        DBuf<uint32_t> d_cstart, d_seeded, d_tile_cnt;
        DBuf<uint64_t> d_keys;
        DBuf<unsigned long long> d_max, d_hist;
        DBuf<int64_t> d_tile_off;
        DBuf<lm_seed_dist_rec> d_recs;
        DBuf<lm_seed_dist_row> d_rows;
        sp_upload(ix, d_coff, coff);
        sp_upload(ix, d_cstart, cstart);
        sp_upload(ix, d_keys, L.keys);
        d_seeded.alloc_exact((size_t)nsel, true, stream);
        d_max.alloc_exact((size_t)nsel, true, stream);
        d_hist.alloc_exact(std::max<size_t>(opt.hist_bins, 1), true, stream);
        d_tile_cnt.alloc_exact((size_t)ntiles + 1, true, stream);
        d_tile_off.alloc_exact((size_t)ntiles + 1, true, stream);
        d_recs.alloc_exact((size_t)nsel);
        SdArgs a{L.ent.p, n, ntiles, d_coff.p, d_cstart.p, opt.min_dist, opt.hist_bins, opt.hist_width, d_max.p, d_seeded.p, d_hist.p,
                 d_tile_cnt.p, d_tile_off.p, nullptr};
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ntiles, 2048));
        int64_t nrows = 0;
        if (n > 0) {
            hipLaunchKernelGGL(k_sd_pass<false>, dim3(grid), dim3(256), (size_t)opt.hist_bins * 4, stream, a);
            HIPCHK(hipGetLastError());
            prim_scan_to_i64(stream, ix->lane[0].main.tmp, d_tile_cnt.p, (size_t)ntiles, d_tile_off.p);
            HIPCHK(hipMemcpyAsync(&nrows, d_tile_off.p + ntiles, sizeof nrows, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
        }
        hipLaunchKernelGGL(k_sd_records, dim3(sp_grid(nsel)), dim3(256), 0, stream, d_keys.p, L.off.p, d_coff.p, d_max.p, d_seeded.p, nsel, d_recs.p);
        HIPCHK(hipGetLastError());
        if (nrows > 0) {
            try {
                d_rows.alloc_exact((size_t)nrows);
            } catch (const DeviceOOM &e) {
                throw DeviceOOM("lm_index_seed_distances: the " + std::to_string(nrows) + " reported rows (24 B each) do not fit on the device beside the "
                                "index and the sorted positions (a larger min_dist reports fewer): " + e.what());
            }
            a.rows = d_rows.p;
            hipLaunchKernelGGL(k_sd_pass<true>, dim3(grid), dim3(256), 0, stream, a);
            HIPCHK(hipGetLastError());
        }
        res->recs.resize((size_t)nsel);
        res->hist.resize(opt.hist_bins);
        res->rows.resize((size_t)nrows);
        if (nsel > 0) HIPCHK(hipMemcpyAsync(res->recs.data(), d_recs.p, (size_t)nsel * sizeof(lm_seed_dist_rec), hipMemcpyDeviceToHost, stream));
        if (opt.hist_bins > 0) HIPCHK(hipMemcpyAsync(res->hist.data(), d_hist.p, (size_t)opt.hist_bins * 8, hipMemcpyDeviceToHost, stream));
        if (nrows > 0) HIPCHK(hipMemcpyAsync(res->rows.data(), d_rows.p, (size_t)nrows * sizeof(lm_seed_dist_row), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    });
    if (st == LM_OK) *out = res.release();
    return st;
}
extern "C" size_t lm_seed_dist_records(const lm_seed_dist *sd, const lm_seed_dist_rec **recs) {
    if (!sd) return 0;
    if (recs) *recs = sd->recs.data();
    return sd->recs.size();
}
extern "C" size_t lm_seed_dist_hist(const lm_seed_dist *sd, const uint64_t **hist) {
    if (!sd) return 0;
    if (hist) *hist = sd->hist.data();
    return sd->hist.size();
}
extern "C" size_t lm_seed_dist_rows(const lm_seed_dist *sd, const lm_seed_dist_row **rows) {
    if (!sd) return 0;
    if (rows) *rows = sd->rows.data();
    return sd->rows.size();
}
extern "C" void lm_seed_dist_free(lm_seed_dist *sd) { delete sd; }

// ---- the HBM image written back to disk -----------------------------------------------------------------------------------
// `lexicmap index` output as the reference lays it out, EXCEPT masks.bin, which is written in this
// build's own LMMASKS1 layout (lexichash's file layout is not in the reference tree): info.toml (lib-index-build.go:1914-1932),
// seeds/chunk_NNN.bin + .idx (kv/kv-data.go:126-602: per mask the distinct k-mers ascending, two per record,
// k-mer deltas and value counts group-varint coded, 7-byte values while there are <= 512 genome batches; the .idx holds the
// first k-mer and offset of every anchor partition present), genomes/batch_NNNN/genomes.bin + .idx (genome/genome.go:217-357),
// genomes.map.bin (lib-index-build.go:649-655).  What it is for here: the GPU-built benchmark sets become reference-format
// indexes, so the loader (lm_index_open) is exercised and timed at their size and its packed image can be compared with the
// one the builder made in HBM.  (The Go `lexicmap search` could read everything but that masks.bin.)
namespace lm {
namespace {
struct OutFile {
    FILE *f = nullptr;
    int64_t n = 0;
    bool bad = false;
    explicit OutFile(const std::string &p) {
        f = fopen(p.c_str(), "wb");
        bad = f == nullptr;
    }
    ~OutFile() {
        if (f) fclose(f);
    }
    void put(const void *p, size_t len) {
        if (!bad && len && fwrite(p, 1, len, f) != len) bad = true;
        n += (int64_t)len;
    }
    void be(uint64_t v, int bytes) {
        uint8_t b[8];
        for (int i = 0; i < bytes; i++) b[i] = (uint8_t)(v >> (8 * (bytes - 1 - i)));
        put(b, (size_t)bytes);
    }
};
inline void push_be(std::vector<uint8_t> &o, uint64_t v, int bytes) {
    for (int i = bytes - 1; i >= 0; i--) o.push_back((uint8_t)(v >> (8 * i)));
}
inline int byte_len(uint64_t v) {
    int n = 1;
    while (n < 8 && (v >> (8 * n)) != 0) n++;
    return n;
}
// control byte + the two numbers in their minimal big-endian widths (util/varint-GB.go:28-46)
inline void push_pair(std::vector<uint8_t> &o, uint64_t a, uint64_t b, uint8_t flags) {
    const int la = byte_len(a), lb = byte_len(b);
    o.push_back((uint8_t)(flags | ((la - 1) << 3) | (lb - 1)));
    push_be(o, a, la);
    push_be(o, b, lb);
}
bool make_dir(const std::string &p) { return mkdir(p.c_str(), 0777) == 0 || errno == EEXIST; }

// one mask's seeds (any order) -> its block of the chunk file (relative offsets) + its .idx records (kmer, rel offset<<1|second)
void encode_mask(std::vector<std::pair<uint64_t, uint64_t>> &kv, int K, int mask_prefix, int anchor_prefix, bool use7,
                 std::vector<uint8_t> &data, std::vector<std::pair<uint64_t, uint64_t>> &idx) {
    data.clear();
    idx.clear();
    std::sort(kv.begin(), kv.end());
    // distinct k-mers: [start, end) runs
    std::vector<size_t> runs;
    for (size_t i = 0; i < kv.size(); i++)
        if (i == 0 || kv[i].first != kv[i - 1].first) runs.push_back(i);
    const size_t nk = runs.size();
    push_be(data, (uint64_t)nk, 8);
    if (nk == 0) return;
    runs.push_back(kv.size());
    const int vb = use7 ? 7 : 8;
    const int shift = (K - mask_prefix - anchor_prefix) << 1;
    const uint64_t amask = ((uint64_t)1 << (anchor_prefix << 1)) - 1;
    uint64_t seen_part = ~(uint64_t)0, prev_second = 0; // previous record's second k-mer (the delta base)
    auto note = [&](uint64_t kmer, bool second, size_t at) { // first k-mer of every anchor partition, in file order
        const uint64_t part = (kmer >> shift) & amask;
        if (part != seen_part) {
            seen_part = part;
            idx.emplace_back(kmer, ((uint64_t)at << 1) | (second ? 1u : 0u));
        }
    };
    for (size_t r = 0; r < nk; r += 2) {
        const bool pair = r + 1 < nk, last = r + 2 >= nk;
        const uint64_t k1 = kv[runs[r]].first, k2 = pair ? kv[runs[r + 1]].first : 0;
        const uint64_t n1 = runs[r + 1] - runs[r], n2 = pair ? runs[r + 2] - runs[r + 1] : 0;
        const size_t at = data.size();
        note(k1, false, at);
        if (pair) note(k2, true, at);
        push_pair(data, k1 - prev_second, pair ? k2 - k1 : 0, (uint8_t)((last ? 128 : 0) | (pair ? 0 : 64)));
        push_pair(data, n1, n2, 0);
        for (size_t i = runs[r]; i < runs[r] + n1 + n2; i++) push_be(data, kv[i].second, vb);
        prev_second = pair ? k2 : k1;
    }
}
} // namespace
} // namespace lm

extern "C" lm_status lm_index_save(lm_index *ix, const char *dir_c, int chunks) {
    using namespace lm;
    if (!ix || !dir_c) return LM_ERR_ARG;
    std::lock_guard<std::mutex> lock(ix->mu);
    const HostIndex &h = ix->host;
    if (h.shard_count > 1) {
        ix->err = "lm_index_save: a shard of an index cannot be saved (open or build it unsharded)";
        return LM_ERR_ARG;
    }
    try {
        HIPCHK(hipSetDevice(ix->device));
        const std::string dir(dir_c);
        const int M = h.M, K = h.k;
        if (chunks < 1) chunks = 1;
        if (chunks > M) chunks = M;
        // info.toml names the number of chunk FILES: ceil(M / ceil(M / chunks)) of them are written (M = 100 masks asked into 16
        // chunks are 15 files of 7 masks), as the reference's writer and the oracle's do
        chunks = (M + (M + chunks - 1) / chunks - 1) / ((M + chunks - 1) / chunks);
        const int bsz = h.genome_batch_size > 0 ? h.genome_batch_size : 5000;
        const int nbatches = std::max(1, h.genome_batches > 0 ? h.genome_batches : (int)((h.genomes.size() + (size_t)bsz - 1) / (size_t)bsz));
        const bool use7 = nbatches <= 512; // kv-data.go:137
        if (!make_dir(dir) || !make_dir(dir + "/seeds") || !make_dir(dir + "/genomes")) throw HipError("lm_index_save: cannot create " + dir);
        // ---- masks.bin (this build's layout, lm_format.cpp) and info.toml
        {
            OutFile f(dir + "/masks.bin");
            f.put("LMMASKS1", 8);
            f.be((uint64_t)K, 1);
            f.be(0, 3);
            f.be((uint64_t)M, 4);
            f.be(0, 8);
            for (int i = 0; i < M; i++) f.be(h.masks[i], 8);
            if (f.bad) throw HipError("lm_index_save: write failed (masks.bin)");
        }
        int64_t gbases = 0;
        for (auto &g : h.genomes) gbases += g.genome_size;
        {
            OutFile f(dir + "/info.toml");
            char t[1024];
            const int n = snprintf(t, sizeof t,
                                   "# Index format\nmain-version = 3\nminor-version = 5\n# LexicHash\nmax-K = %d\nmasks = %d\nrand-seed = %lld\n"
                                   "# Seed distance\nmax-seed-dist = %d\nseed-dist-in-desert = %d\n# Seeds (k-mer-value data) files\nchunks = %d\n"
                                   "index-partitions = %d\n# Input genomes\ninput-genomes = %lld\ninput-bases = %lld\n# Genome data\ngenomes = %lld\n"
                                   "genome-batch-size = %d\ngenome-batches = %d\ncontig-interval = %d\n",
                                   K, M, (long long)h.rand_seed, h.max_seed_dist, h.seed_dist_in_desert, chunks, 1 << (2 * h.anchor_prefix), (long long)(h.input_genomes > 0 ? h.input_genomes : (int64_t)h.genomes.size()),
                                   (long long)(h.total_bases > 0 ? h.total_bases : gbases), (long long)h.genomes.size(), bsz, nbatches,
                                   h.contig_interval);
            f.put(t, (size_t)n);
            if (f.bad) throw HipError("lm_index_save: write failed (info.toml)");
        }
        // ---- genomes: the batches (5000 records each unless the set was built with another batch size) in dense order, bases
        // straight from the 2-bit store in HBM
        {
            OutFile fmap(dir + "/genomes.map.bin");
            std::vector<uint8_t> bits;
            for (int b = 0; b < nbatches; b++) {
                char nm[64];
                snprintf(nm, sizeof nm, "/genomes/batch_%04d", b);
                if (!make_dir(dir + nm)) throw HipError("lm_index_save: cannot create the genome batch directory");
                OutFile fg(dir + nm + "/genomes.bin"), fi(dir + nm + "/genomes.bin.idx");
                fg.put(".genomes", 8);
                fg.be(0, 1);
                fg.be(1, 1);
                fg.be(0, 6);
                std::vector<const HostGenome *> members;
                for (auto &g : h.genomes)
                    if ((int)(g.bg >> 17) == b) members.push_back(&g);
                std::sort(members.begin(), members.end(), [](const HostGenome *x, const HostGenome *y) { return x->bg < y->bg; });
                fi.put(".genomei", 8);
                fi.be(0, 1);
                fi.be(1, 1);
                fi.be(0, 6);
                fi.be((uint64_t)b, 4);
                fi.be((uint64_t)members.size(), 4);
                for (const HostGenome *g : members) {
                    fi.be((uint64_t)fg.n, 8);
                    fi.be((uint64_t)g->len, 4);
                    fg.be(g->id.size(), 2);
                    fg.put(g->id.data(), g->id.size());
                    fg.be((uint64_t)g->genome_size, 4);
                    fg.be((uint64_t)g->len, 4);
                    fg.be((uint64_t)g->nseqs, 4);
                    for (int s = 0; s < g->nseqs; s++) {
                        fg.be((uint64_t)g->seq_sizes[s], 4);
                        fg.be(g->seq_ids[s].size(), 2);
                        fg.put(g->seq_ids[s].data(), g->seq_ids[s].size());
                    }
                    const size_t nb = ((size_t)g->len + 3) >> 2;
                    bits.resize(nb);
                    {
                        const size_t l = (size_t)(g - ix->host.genomes.data());
                        if (!ix->g_hhost.empty() && ix->g_hhost[l]) memcpy(bits.data(), ix->g_hhost[l], nb); // host-resident: read where it lives
                        else HIPCHK(hipMemcpy(bits.data(), ix->d_gbits.p + g->bits_off, nb, hipMemcpyDeviceToHost));
                    }
                    fg.be(nb, 4);
                    fg.be((uint64_t)g->len, 4);
                    fg.put(bits.data(), nb);
                    fmap.be(g->id.size(), 2);
                    fmap.put(g->id.data(), g->id.size());
                    fmap.be(g->bg, 8);
                }
                if (fg.bad || fi.bad) throw HipError("lm_index_save: write failed (genomes)");
            }
            if (fmap.bad) throw HipError("lm_index_save: write failed (genomes.map.bin)");
        }
        // ---- genomes.chunks.bin (lib-index-build.go:1787-1808): per split genome the number of its chunks and their keys, in
        // chunk order; written (empty when no genome was split) so that the saved index is complete for the reference's reader
        {
            std::map<int, std::vector<std::pair<int, uint64_t>>> lists; // list number -> (chunk index, key)
            for (const auto &kv : h.chunk_of) lists[kv.second.list].emplace_back(kv.second.idx, kv.first);
            OutFile fc(dir + "/genomes.chunks.bin");
            for (auto &li : lists) {
                if (li.second.size() <= 1) continue;
                std::sort(li.second.begin(), li.second.end());
                fc.be((uint64_t)li.second.size(), 8);
                for (const auto &e : li.second) fc.be(e.second, 8);
            }
            if (fc.bad) throw HipError("lm_index_save: write failed (genomes.chunks.bin)");
        }
        // ---- seeds: masks split evenly over the chunk files (lib-index-build.go:1861-1889)
        std::vector<int64_t> md_off((size_t)2 * M + 1), out_off((size_t)2 * M + 1);
        HIPCHK(hipMemcpy(md_off.data(), ix->d_md_off.p, md_off.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out_off.data(), ix->d_out_off.p, out_off.size() * 8, hipMemcpyDeviceToHost));
        DBuf<uint64_t> dk, dv;
        const int per = (M + chunks - 1) / chunks;
        for (int c = 0, m0 = 0; m0 < M; c++, m0 += per) {
            const int m1 = std::min(M, m0 + per);
            // every list of the chunk's masks unpacked into one buffer, one copy to the host
            const int64_t s0 = md_off[(size_t)2 * m0], s1 = md_off[(size_t)2 * m1], ns = s1 - s0;
            std::vector<uint64_t> hk((size_t)ns), hv((size_t)ns);
            if (ns > 0) {
                dk.ensure((size_t)ns);
                dv.ensure((size_t)ns);
                for (int md = 2 * m0; md < 2 * m1; md++) {
                    const int64_t nm = md_off[(size_t)md + 1] - md_off[(size_t)md];
                    if (nm > 0)
                        hipLaunchKernelGGL(lm::k_sp_dump_list, dim3(lm::sp_grid(nm)), dim3(256), 0, ix->lane[0].main.st, ix->view, (uint32_t)md, nm,
                                           dk.p + (md_off[(size_t)md] - s0), dv.p + (md_off[(size_t)md] - s0));
                }
                HIPCHK(hipMemcpyAsync(hk.data(), dk.p, (size_t)ns * 8, hipMemcpyDeviceToHost, ix->lane[0].main.st));
                HIPCHK(hipMemcpyAsync(hv.data(), dv.p, (size_t)ns * 8, hipMemcpyDeviceToHost, ix->lane[0].main.st));
                HIPCHK(hipStreamSynchronize(ix->lane[0].main.st));
            }
            const int64_t o0 = out_off[(size_t)2 * m0], o1 = out_off[(size_t)2 * m1], no = o1 - o0;
            std::vector<uint64_t> ok((size_t)no), ov((size_t)no);
            if (no > 0) {
                HIPCHK(hipMemcpy(ok.data(), ix->d_out_kmers.p + o0, (size_t)no * 8, hipMemcpyDeviceToHost));
                HIPCHK(hipMemcpy(ov.data(), ix->d_out_vals.p + o0, (size_t)no * 8, hipMemcpyDeviceToHost));
            }
            // encode the masks on the host threads, then lay the blocks out and fix the offsets up
            const int nm = m1 - m0;
            std::vector<std::vector<uint8_t>> blocks((size_t)nm);
            std::vector<std::vector<std::pair<uint64_t, uint64_t>>> recs((size_t)nm);
            std::atomic<int> next{0};
            auto work = [&]() {
                std::vector<std::pair<uint64_t, uint64_t>> kv;
                for (int j; (j = next.fetch_add(1)) < nm;) {
                    const int m = m0 + j;
                    kv.clear();
                    for (int64_t i = md_off[(size_t)2 * m] - s0; i < md_off[(size_t)2 * m + 2] - s0; i++) kv.emplace_back(hk[(size_t)i], hv[(size_t)i]);
                    for (int64_t i = out_off[(size_t)2 * m] - o0; i < out_off[(size_t)2 * m + 2] - o0; i++) kv.emplace_back(ok[(size_t)i], ov[(size_t)i]);
                    encode_mask(kv, K, h.mask_prefix, h.anchor_prefix, use7, blocks[(size_t)j], recs[(size_t)j]);
                }
            };
            {
                const int nth = std::max(1, std::min<int>(16, (int)std::thread::hardware_concurrency()));
                std::vector<std::thread> th;
                for (int t = 1; t < nth; t++) th.emplace_back(work);
                work();
                for (auto &t : th) t.join();
            }
            char nmf[64];
            snprintf(nmf, sizeof nmf, "/seeds/chunk_%03d.bin", c);
            OutFile fd(dir + nmf), fx(dir + nmf + ".idx");
            fd.put(".kv-data", 8);
            fd.be(1, 1);
            fd.be(1, 1);
            fd.be((uint64_t)K, 1);
            fd.be(use7 ? 1 : 0, 1);
            fd.be(0, 4);
            fd.be((uint64_t)m0, 8);
            fd.be((uint64_t)nm, 8);
            fx.put(".kvindex", 8);
            fx.be(1, 1);
            fx.be(1, 1);
            fx.be((uint64_t)K, 1);
            fx.be((uint64_t)h.mask_prefix, 1);
            fx.be((uint64_t)h.anchor_prefix, 1);
            fx.be(use7 ? 1 : 0, 1);
            fx.be(0, 2);
            fx.be((uint64_t)m0, 8);
            fx.be((uint64_t)nm, 8);
            for (int j = 0; j < nm; j++) {
                const int64_t at = fd.n; // the mask's block starts with its k-mer count
                fd.put(blocks[(size_t)j].data(), blocks[(size_t)j].size());
                const auto &r = recs[(size_t)j];
                if (r.empty()) {
                    fx.be(0, 8);
                    continue;
                }
                // record 0: (number of records, offset of the mask's first record << 1), then one per anchor partition present
                fx.be((uint64_t)r.size() + 1, 8);
                fx.be((uint64_t)r.size() + 1, 8);
                fx.be((uint64_t)(at + 8) << 1, 8);
                for (auto &e : r) {
                    fx.be(e.first, 8);
                    fx.be((((e.second >> 1) + (uint64_t)at) << 1) | (e.second & 1), 8);
                }
            }
            if (fd.bad || fx.bad) throw HipError("lm_index_save: write failed (seeds)");
        }
        return LM_OK;
    } catch (const std::exception &e) {
        ix->err = e.what();
        return LM_ERR_HIP;
    }
}
