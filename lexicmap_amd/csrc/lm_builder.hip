// lm_builder.hip — the seed index built on the GPU.  One seed pipeline with two front ends:
//   * lm_index_build_synthetic(_ex): a synthetic genome set generated directly in HBM (bench / large-scale test input).  It
//     exists because the benchmark configurations (10k x 5 Mb genomes and up) cannot be built by any CPU tool on a fresh box
//     within minutes, and nothing persists on the GPU box.  Genomes: procedural i.i.d. ACGT ancestors per family; members
//     are substituted (rate U(0,max_div)) and indel-shifted copies; single contig; stored 2-bit MSB-first like
//     genome/genome.go:1471-1508.  A sharded set is numbered without a table: local genome l is genome l * shard_count + rank.
//   * lm_index_builder_*: caller-supplied genomes of any length, with several contigs and skip regions, added one by one
//     (planner of records, spacers, skip regions, keys, shards: lm_build_plan.h), or added to a resident index (_extend).
// A front end validates its settings, sets up the header and the masks (builder_header), puts the 2-bit records into one
// store and describes them in HostIndex::genomes; build_seed_index does the rest for both, with the same kernels.  What it
// produces has the same structure as a reference-built index (lib-index-build.go):
//   * normal seeds: EXACT LexicHash capture per record — for every mask the argmin of mask^kmer over both strands, all
//     occurrences, low-complexity captures dropped (lib-index-build.go:1028-1046); k-mers that overlap a skip region are
//     left out, and a mask whose p-base prefix no k-mer of the record shares captures the argmin over ALL k-mers
//     (lexichash MaskKnownDistinctPrefixes(..., checkShorterPrefix = true), lib-index-build.go:1028)
//   * seed-desert filling as the reference does it (lib-index-build.go:1094-1407): every gap >= max_desert between
//     neighbouring seeds is filled every seed_dist bases with the nearest non-low-complexity k-mer (scan 25 up-, then 24
//     downstream, + strand before - strand) that is the capture of a mask when the window [pre - 1000, pos + 1000 + k)
//     alone is masked, stored under the last mask capturing it (tests/test_gpu_builder.py: every mask's list equals what
//     the oracle's writer stores for the same genomes)
//   * reversed (suffix) seeds for every normal and desert seed (lib-index-build.go:776-890)
//   * seed values batch:17|genome:17|pos:28|strand:1|reversed:1, per-mask arrays sorted by k-mer
// The search kernels and the parity tests never depend on this file: parity uses indexes written in the reference's
// on-disk format by the oracle's writer.
#include <cmath>
#include <cstring>

#include "lm_internal.h"
#include "lm_prims.h"
#include "lm_build_plan.h"
#include "lm_mask_plan.h"
#include "lm_join_plan.h"

namespace lm {

static inline void bsync(lm_index *ix) {
    hipError_t e = hipStreamSynchronize(ix->lane[0].main.st);
    if (e != hipSuccess) throw HipError(std::string("builder sync: ") + hipGetErrorString(e));
}

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ uint64_t hash3(uint64_t a, uint64_t b, uint64_t c) {
    return mix64(mix64(mix64(a) ^ b) ^ c);
}

struct SynthDev {
    uint64_t seed;
    int64_t genomes;  // whole set
    int32_t genome_len, families;
    double max_div;
    int32_t shard_rank, shard_count;
    int64_t nlocal;
    int32_t nblk;     // 512-base blocks per genome
    int64_t gbytes;   // padded bytes per genome
};

__device__ __forceinline__ int64_t global_genome(const SynthDev &sp, int64_t local) {
    return sp.shard_count > 1 ? local * sp.shard_count + sp.shard_rank : local;
}
__device__ __forceinline__ double genome_div(const SynthDev &sp, int64_t g) {
    if (g < sp.families) return 0.0;
    return sp.max_div * ((double)(hash3(sp.seed, 0xD1Full, (uint64_t)g) >> 11) * (1.0 / 9007199254740992.0));
}

// cumulative indel shift per 512-base block
__global__ void k_synth_shifts(SynthDev sp, int16_t *__restrict__ shifts) {
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < sp.nlocal; l += (int64_t)gridDim.x * blockDim.x) {
        int64_t g = global_genome(sp, l);
        double d = genome_div(sp, g);
        // indel events at a tenth of the substitution rate: 8 trials per block
        uint32_t thr = (uint32_t)(fmin(1.0, d * 0.1 * 512.0 / 8.0) * 4294967295.0);
        int sh = 0;
        for (int b = 0; b < sp.nblk; b++) {
            if (g >= sp.families) {
                uint64_t h = hash3(sp.seed, 0x5117ull + (uint64_t)g, (uint64_t)b);
                for (int t = 0; t < 8; t++) {
                    uint64_t hh = mix64(h + t);
                    if ((uint32_t)hh < thr) sh += (hh >> 63) ? 1 : -1;
                }
                if (sh > 30000) sh = 30000;
                if (sh < -30000) sh = -30000;
            }
            shifts[l * sp.nblk + b] = (int16_t)sh;
        }
    }
}

__device__ __forceinline__ uint32_t synth_base(const SynthDev &sp, int64_t g, int64_t i, int sh, uint32_t sub_thr) {
    uint64_t f = (uint64_t)(g % sp.families);
    uint32_t anc = (uint32_t)(hash3(sp.seed, 0xA11Cull + f, (uint64_t)(i + sh)) >> 17) & 3u;
    if (g >= sp.families) {
        uint64_t h = hash3(sp.seed, 0x5B5ull + (uint64_t)g, (uint64_t)i);
        if ((uint32_t)h < sub_thr) anc = (anc + 1u + (uint32_t)((h >> 40) % 3u)) & 3u;
    }
    return anc;
}

// one lane per packed byte (4 bases, first base in bits 7-6)
__global__ void k_synth_genomes(SynthDev sp, const int16_t *__restrict__ shifts, uint8_t *__restrict__ gbits) {
    int64_t nb = ((int64_t)sp.genome_len + 3) >> 2;
    int64_t total = sp.nlocal * nb;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t l = t / nb, by = t % nb;
        int64_t g = global_genome(sp, l);
        uint32_t thr = (uint32_t)(genome_div(sp, g) * 4294967295.0);
        uint32_t v = 0;
        for (int j = 0; j < 4; j++) {
            int64_t i = by * 4 + j;
            uint32_t b = 0;
            if (i < sp.genome_len) b = synth_base(sp, g, i, shifts[l * sp.nblk + (i >> 9)], thr);
            v = (v << 2) | b;
        }
        gbits[l * sp.gbytes + by] = (uint8_t)v;
    }
}

// 31-mer at base position pos of a packed genome: two ALIGNED 64-bit loads + funnel shift (genomes start on 8-byte
// boundaries and are padded by 16 bytes; an unaligned 8-byte memcpy compiles to byte loads)
__device__ __forceinline__ uint64_t packed_kmer(const uint8_t *gb, int64_t pos, int K) {
    const int64_t byte = pos >> 2;
    const uint64_t *p = (const uint64_t *)(gb + (byte & ~7ll));
    const uint64_t H = __builtin_bswap64(p[0]), L = __builtin_bswap64(p[1]);
    const int o = (int)(byte & 7) * 8 + (int)(pos & 3) * 2; // 0..62
    const uint64_t v = o ? ((H << o) | (L >> (64 - o))) : H;
    return v >> (64 - (K << 1));
}

struct MaskTab {
    const uint64_t *masks;
    const int32_t *pfx_first;
    int K, p, M;
};

__device__ __forceinline__ int closest_mask(const MaskTab &mt, uint64_t x) {
    uint64_t pf = x >> ((mt.K - mt.p) << 1);
    int minj = -1;
    uint64_t minh = ~0ull;
    for (int j = mt.pfx_first[pf]; j < mt.pfx_first[pf + 1]; j++) {
        uint64_t h = mt.masks[j] ^ x;
        if (h < minh) {
            minh = h;
            minj = j;
        }
    }
    return minj;
}

// the p-base prefixes (p <= 16) of the k-mer at `pos` and of its reverse complement, from one 32-base window of the 2-bit
// genome: all the sweep below needs for the ~16 000 : 1 window k-mers that do not share the candidate's prefix
__device__ __forceinline__ void kmer_prefixes(const uint8_t *gb, int64_t pos, int K, int p, uint32_t *fwd, uint32_t *rc) {
    const int64_t byte = pos >> 2;
    const uint64_t *q = (const uint64_t *)(gb + (byte & ~7ll));
    const uint64_t H = __builtin_bswap64(q[0]), L = __builtin_bswap64(q[1]);
    const int o = (int)(byte & 7) * 8 + (int)(pos & 3) * 2; // 0..62
    const uint64_t v = o ? ((H << o) | (L >> (64 - o))) : H; // 32 bases from pos, left aligned
    *fwd = (uint32_t)(v >> (64 - 2 * p));
    const uint32_t last = (uint32_t)(v >> (64 - 2 * K)) & ((1u << (2 * p)) - 1u); // the last p bases of the k-mer
    uint32_t y = __builtin_bitreverse32(~last);                                    // complement, reverse the bits ...
    y = ((y >> 1) & 0x55555555u) | ((y & 0x55555555u) << 1);                       // ... and put the base pairs back in order
    *rc = y >> (32 - 2 * p);
}
// the capture test of a desert candidate x (k_desert_fill_g), by the 64 lanes of a wavefront: the last mask for which x
// attains the minimum over the nk k-mers of the window from wstart, or -1
__device__ __forceinline__ int desert_capturing_mask(const MaskTab &mt, const uint8_t *gb, int64_t wstart, int nk, uint64_t x,
                                                     int lane) {
    const int shift = (mt.K - mt.p) << 1;
    const uint32_t pf = (uint32_t)(x >> shift);
    const int j0 = mt.pfx_first[pf], j1 = mt.pfx_first[pf + 1];
    if (j0 >= j1) return -1;
    // one sweep of the window for all masks of the prefix (1 .. 32: lm_mask_plan.h refuses a set with more): bit j - j0 = x is
    // beaten for mask j
    uint32_t beaten = 0;
    for (int w = lane; w < nk; w += 64) {
        uint32_t pfw, prc;
        kmer_prefixes(gb, wstart + w, mt.K, mt.p, &pfw, &prc);
        if (pfw == pf || prc == pf) {
            const uint64_t f = packed_kmer(gb, wstart + w, mt.K), r = lm_revcomp(f, mt.K);
            for (int j = j0; j < j1 && j - j0 < 32; j++) {
                const uint64_t mk = mt.masks[j], hx = mk ^ x;
                if ((pfw == pf && (mk ^ f) < hx) || (prc == pf && (mk ^ r) < hx)) beaten |= 1u << (j - j0);
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) beaten |= (uint32_t)__shfl_xor((int)beaten, o, 64);
    int im = -1;
    for (int j = j0; j < j1 && j - j0 < 32; j++)
        if (!((beaten >> (j - j0)) & 1u)) im = j; // x attains the window's minimum for mask j; the last such mask is recorded
    return im;
}

// reversed copies of seeds [from, to)
__global__ void k_reverse_seeds(MaskTab mt, unsigned long long from, unsigned long long to, uint16_t *__restrict__ s_mask,
                                uint64_t *__restrict__ s_kmer, uint64_t *__restrict__ s_val,
                                unsigned long long *__restrict__ counter, unsigned long long cap) {
    for (unsigned long long t = from + (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; t < to;
         t += (unsigned long long)gridDim.x * blockDim.x) {
        uint64_t rev = lm_reverse(s_kmer[t], mt.K);
        int m = closest_mask(mt, rev);
        unsigned long long o = atomicAdd(counter, 1ull);
        if (o < cap && m >= 0) {
            s_mask[o] = (uint16_t)m;
            s_kmer[o] = rev;
            s_val[o] = s_val[t] | 1ull;
        }
    }
}

__global__ void k_fetch_bases(const uint8_t *__restrict__ gb, int64_t start, int64_t len, uint8_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t p = start + i;
        out[i] = (uint8_t)("ACGT"[(gb[p >> 2] >> ((3 - (p & 3)) << 1)) & 3]);
    }
}

static int gridn(int64_t n, int block = 256) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 262144) g = 262144;
    return (int)g;
}

static int mask_prefix_of(int M) { return std::max(1, (int)(std::log2((double)M) / 2)); }

// host-side mask set with the structure of lexicmap masks (docs/content/usage/utils/masks.md:69-110): all p-prefixes
// present, M-4^p extra masks on distinct prefixes differing from their twin at base p+1, sorted.
static void gen_masks(int k, int M, uint64_t seed, std::vector<uint64_t> &out) {
    int p = mask_prefix_of(M);
    int64_t np = (int64_t)1 << (2 * p);
    int lowbits = (k - p) << 1;
    uint64_t lowmask = (1ull << lowbits) - 1;
    uint64_t st = seed * 0x2545F4914F6CDD1Dull + 0x9E37ull;
    auto next = [&]() {
        st += 0x9E3779B97F4A7C15ull;
        return mix64(st);
    };
    out.clear();
    for (int64_t i = 0; i < np && (int)out.size() < M; i++) {
        uint64_t m;
        do m = ((uint64_t)i << lowbits) | (next() & lowmask);
        while (lm_dust(m, k));
        out.push_back(m);
    }
    int extra = M - (int)out.size();
    std::vector<int64_t> perm(np);
    for (int64_t i = 0; i < np; i++) perm[i] = i;
    for (int j = 0; j < extra; j++) {
        int64_t r = j + (int64_t)(next() % (uint64_t)(np - j));
        std::swap(perm[j], perm[r]);
        uint64_t twin_base = (out[perm[j]] >> (lowbits - 2)) & 3;
        uint64_t m;
        do m = ((uint64_t)perm[j] << lowbits) | (next() & lowmask);
        while (((m >> (lowbits - 2)) & 3) == twin_base || lm_dust(m, k));
        out.push_back(m);
    }
    std::sort(out.begin(), out.end());
}

// =====================================================================================================================
// The seed kernels.  Geometry comes from tables, so that one set of kernels serves records of any length: g_off / g_len /
// g_bg per record and a CSR of skip regions (spacers between contigs, runs of N; empty for a synthetic set).
struct GenomeTab {
    const int64_t *g_off;   // [nlocal] byte offset of the record in the store
    const int32_t *g_len;   // [nlocal] bases
    const uint64_t *g_bg;   // [nlocal] batch << 17 | index
    const int32_t *reg_off; // [nlocal + 1] CSR of the skip regions of every record
    const int32_t *reg_s, *reg_e; // inclusive, ascending, disjoint
};

// does the k-mer starting at pos overlap a skip region, i.e. is pos inside one of the intervals [s - K + 1, e]
// (the masking's skip-region cursor and the desert filling's interval test: one predicate for ascending disjoint regions)
__device__ __forceinline__ bool kmer_skipped(const int32_t *__restrict__ rs, const int32_t *__restrict__ re, int n, int pos, int K) {
    if (n == 0) return false;
    int lo = 0, hi = n; // first region that ends at or behind pos
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (re[mid] < pos) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && pos + K - 1 >= rs[lo];
}

// ASCII contigs of one record -> its 2-bit concatenation (contigs + spacers of A), MSB first; one lane per packed byte.
// src_off: where contig c starts in `ascii`; dst_off: where it starts in the concatenation; every byte of the record is written
__global__ void k_pack_record(const uint8_t *__restrict__ ascii, const int64_t *__restrict__ src_off, const int32_t *__restrict__ dst_off,
                              const int32_t *__restrict__ clen, int nc, int32_t len, uint8_t *__restrict__ out) {
    const int64_t nb = ((int64_t)len + 3) >> 2;
    for (int64_t by = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; by < nb; by += (int64_t)gridDim.x * blockDim.x) {
        uint32_t v = 0;
        int lo = 0, hi = nc; // the last contig that starts at or before the byte's first base
        const int32_t i0 = (int32_t)(by << 2);
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (dst_off[mid] <= i0) lo = mid;
            else hi = mid;
        }
        int c = lo;
        for (int j = 0; j < 4; j++) {
            const int32_t i = i0 + j;
            uint32_t b = 0;
            if (i < len) {
                while (c + 1 < nc && dst_off[c + 1] <= i) c++;
                const int32_t r = i - dst_off[c];
                if (r < clen[c]) b = build_base_code(ascii[src_off[c] + r]); // (else: inside the spacer behind contig c)
            }
            v = (v << 2) | b;
        }
        out[by] = (uint8_t)v;
    }
}

// LexicHash capture of one record by one workgroup, all phases in one launch.  LDS = true: the per-mask minima live in LDS
// (M x 8 B = 160 KB for the default 20000 masks: the whole LDS of a CU) instead of a global table hammered with atomics;
// false (more masks than a CU's LDS holds): in ghash[block][M].  CSR = false: the masks of a p-base prefix are found without
// a table in memory: in a lexicmap mask set every prefix has one mask and some have two
// (docs/content/usage/utils/masks.md:69-110), so first(pf) = pf + #doubled prefixes below pf: a 4^p-bit map + per-word counts
// (2.5 KB).  CSR = true (a caller's or an opened index's set with three or more masks on some prefix): from the prefix table
// mt.pfx_first, copied to LDS where the host found room for it (TLDS).  Only phase 1 and the prefix part of phase 2 differ.
// Phase 1: ds_min_u64 of mask^kmer over the k-mers sharing a mask's prefix, k-mers that overlap a skip region left out.
// Phase 1b, the missing-prefix rule: a mask whose minimum is still untouched takes the argmin over ALL
// k-mers of both strands - one lane per such mask, the k-mers cut 64 at a time and passed round the wavefront; the lane also
// counts the occurrences of its minimum and keeps the first.  A wavefront without such a mask skips the sweep, so a genome
// in which every prefix occurs (5 Mb: 600 k-mers per prefix) pays one pass over the minima.  Phase 2: every k-mer equal to
// its mask's minimum is emitted (all occurrences, lib-index-build.go:1028-1046), low-complexity captures dropped, plus the
// captures of phase 1b from what their lanes kept (a k-mer that occurs more than once is looked up again).
// miss_pos / miss_cnt: [block][M] scratch, (pos << 1 | strand) + 1 of the first occurrence (0: captured in phase 1 or not at
// all) and the number of occurrences.
// a minimum as every lane of the workgroup sees it after a barrier: in global memory (LDS = false) the atomics of phase 1 went
// to L2, so the read must not be served from a line an earlier plain load left in the CU's vector cache
template <bool LDS> __device__ __forceinline__ unsigned long long cap_min_load(const unsigned long long *p) {
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// The masks [j0, j0 + nj) of the p-base prefix pf (a macro: the CSR = false instantiations keep the statements, and so the code,
// they had before there was a second way).  CSR = false: from the doubled-prefix map, which needs every prefix once or
// twice (every generated set).  CSR = true: from the prefix table pt, 4^p + 1 entries (any set lm_mask_plan.h accepts: up to
// 32 masks on a prefix), which is mt.pfx_first in global memory or the workgroup's copy of it in LDS (TLDS).
#define LM_PREFIX_MASKS(pf)                                                                                                \
    const unsigned long long w = CSR ? 0ull : bm[(pf) >> 6];                                                               \
    const int j0 = CSR ? pt[(pf)] : (int)((pf) + bc[(pf) >> 6] + (uint32_t)__popcll(w & ((1ull << ((pf) & 63)) - 1)));      \
    const int nj = CSR ? pt[(pf) + 1] - j0 : 1 + (int)((w >> ((pf) & 63)) & 1ull);
// LDS of the CSR instantiations: the minima [M] (LDS), the wave totals of phase 2 [16], the prefix table [4^p + 1] (TLDS)
// KM = true (genome screening, lm_screen_capture): only the captured k-mer of every mask is wanted - the minimum xor its mask,
// 0 where the record has no k-mer or the capture is of low complexity.  The launch ends after phase 1b and writes
// s_kmer[block][M]; miss_pos / miss_cnt, the other staging arrays and the counters are not touched (null).  KM = false is the
// kernel as it was: every added statement is under a compile-time `if (KM)`.
template <bool LDS, bool CSR, bool TLDS, bool KM = false>
__global__ __launch_bounds__(1024) void k_capture_g(GenomeTab gt, MaskTab mt, const uint8_t *__restrict__ gbits, int64_t l0,
                                                    const uint64_t *__restrict__ dbl_map, const uint32_t *__restrict__ dbl_cnt,
                                                    unsigned long long *__restrict__ ghash, uint32_t *__restrict__ miss_pos,
                                                    uint32_t *__restrict__ miss_cnt, uint16_t *__restrict__ s_mask,
                                                    uint64_t *__restrict__ s_kmer, uint64_t *__restrict__ s_val,
                                                    unsigned long long *__restrict__ counter, unsigned long long cap,
                                                    uint64_t *__restrict__ pos_keys, unsigned long long *__restrict__ pos_counter,
                                                    unsigned long long pos_cap, unsigned long long *__restrict__ clk) {
    extern __shared__ unsigned long long lds_dyn[];
    const int c = blockIdx.x;
    const int nw = ((1 << (2 * mt.p)) + 63) >> 6;
    const bool stamp = clk && blockIdx.x == 0 && threadIdx.x == 0; // LM_DEBUG: the phases of the chunk's first record (100-MHz clock)
    if (stamp) clk[0] = wall_clock64();
    unsigned long long *hs = LDS ? lds_dyn : ghash + (int64_t)c * mt.M;  // [M]
    unsigned long long *bm = LDS ? lds_dyn + mt.M : lds_dyn;             // [nw]  (CSR: the wave totals and the table start here)
    uint32_t *bc = (uint32_t *)(bm + nw);                                // [nw]
    int32_t *pl = (int32_t *)bm + 16;                                    // [4^p + 1]  (TLDS)
    const int32_t *pt = TLDS ? pl : mt.pfx_first;
    uint32_t *mp = miss_pos + (int64_t)c * mt.M, *mc = miss_cnt + (int64_t)c * mt.M;
    const int64_t l = l0 + c;
    const uint8_t *gb = gbits + gt.g_off[l];
    const int npos = gt.g_len[l] - mt.K + 1;
    const int32_t *rs = gt.reg_s + gt.reg_off[l], *re = gt.reg_e + gt.reg_off[l];
    const int nreg = gt.reg_off[l + 1] - gt.reg_off[l];
    const int shift = (mt.K - mt.p) << 1;
    const int lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < mt.M; i += blockDim.x) hs[i] = ~0ull;
    if (!CSR)
        for (int i = threadIdx.x; i < nw; i += blockDim.x) {
            bm[i] = dbl_map[i];
            bc[i] = dbl_cnt[i];
        }
    if (TLDS)
        for (int i = threadIdx.x; i <= (1 << (2 * mt.p)); i += blockDim.x) pl[i] = mt.pfx_first[i];
    __syncthreads();
    for (int pos = threadIdx.x; pos < npos; pos += blockDim.x) {
        if (kmer_skipped(rs, re, nreg, pos, mt.K)) continue;
        const uint64_t fwd = packed_kmer(gb, pos, mt.K);
        const uint64_t rc = lm_revcomp(fwd, mt.K);
#pragma unroll
        for (int s = 0; s < 2; s++) {
            const uint64_t x = s ? rc : fwd;
            const uint32_t pf = (uint32_t)(x >> shift);
            LM_PREFIX_MASKS(pf)
            for (int j = j0; j < j0 + nj; j++) {
                const unsigned long long h = mt.masks[j] ^ x;
                if (h < hs[j]) atomicMin(&hs[j], h);
            }
        }
    }
    __syncthreads();
    if (stamp) clk[1] = wall_clock64();
    // ---- phase 1b: masks whose prefix does not occur in the record (every lane owns the masks threadIdx.x + i * blockDim.x:
    // nobody else reads or writes their minima here)
    for (int r0 = 0; r0 < mt.M; r0 += blockDim.x) {
        const int j = r0 + threadIdx.x;
        const bool miss = j < mt.M && cap_min_load<LDS>(&hs[j]) == ~0ull;
        if (!__any(miss)) {
            if (!KM && j < mt.M) mp[j] = 0;
            continue;
        }
        const unsigned long long mk = miss ? mt.masks[j] : 0ull;
        unsigned long long best = ~0ull;
        uint32_t bcode = 0, cnt = 0;
        for (int base = 0; base < npos; base += 64) {
            const int pos = base + lane;
            const bool valid = pos < npos && !kmer_skipped(rs, re, nreg, pos, mt.K);
            uint64_t f = 0, r = 0;
            if (valid) {
                f = packed_kmer(gb, pos, mt.K);
                r = lm_revcomp(f, mt.K);
            }
            unsigned long long vm = __ballot(valid);
            while (vm) {
                const int t = __builtin_amdgcn_readfirstlane(__ffsll((long long)vm) - 1);
                vm &= vm - 1;
                const uint64_t ff = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(f >> 32), t) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)f, t);
                const uint64_t rr = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(r >> 32), t) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)r, t);
                const uint32_t code = (uint32_t)(base + t) << 1;
                unsigned long long h = mk ^ ff;
                if (h < best) {
                    best = h;
                    bcode = code;
                    cnt = 1;
                } else if (h == best) cnt++;
                h = mk ^ rr;
                if (h < best) {
                    best = h;
                    bcode = code | 1u;
                    cnt = 1;
                } else if (h == best) cnt++;
            }
        }
        if (j < mt.M) {
            const bool got = miss && best != ~0ull;
            if (!KM) {
                mp[j] = got ? bcode + 1u : 0u;
                mc[j] = got ? cnt : 0u;
            }
            if (got) hs[j] = best;
        }
    }
    if (!LDS) __threadfence();
    __syncthreads();
    if (stamp) clk[2] = wall_clock64();
    if (KM) {
        for (int j = threadIdx.x; j < mt.M; j += blockDim.x) {
            const unsigned long long hj = cap_min_load<LDS>(&hs[j]);
            uint64_t x = hj == ~0ull ? 0ull : hj ^ mt.masks[j];
            if (x != 0 && lm_low_complexity(x, mt.K)) x = 0;
            s_kmer[(int64_t)c * mt.M + j] = x;
        }
        return;
    }
    const uint64_t bg = gt.g_bg[l];
    // ---- phase 2: count, reserve ONE contiguous range of the staging arrays for the record (a per-capture atomic on the
    // shared counter costs more than the whole sweep), write
    uint32_t *wsum = CSR ? (uint32_t *)bm : bc + nw; // [16] wave totals
    __shared__ unsigned long long base_seed, base_pos;
    uint32_t mine = 0;
    for (int sweep = 0; sweep < 2; sweep++) {
        unsigned long long o = 0, po = 0;
        if (sweep == 1) {
            uint32_t incl = mine;
            const int wave = threadIdx.x >> 6;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t v = __shfl_up(incl, d);
                if (lane >= d) incl += v;
            }
            if (lane == 63) wsum[wave] = incl;
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (int w2 = 0; w2 < (int)(blockDim.x >> 6); w2++) {
                if (w2 < wave) before += wsum[w2];
                all += wsum[w2];
            }
            if (threadIdx.x == 0) {
                base_seed = atomicAdd(counter, (unsigned long long)all);
                base_pos = atomicAdd(pos_counter, (unsigned long long)all);
            }
            __syncthreads();
            o = base_seed + before + (incl - mine);
            po = base_pos + before + (incl - mine);
        }
        auto emit = [&](int j, uint64_t x, uint32_t code) { // code = pos << 1 | strand
            if (o < cap) {
                s_mask[o] = (uint16_t)j;
                s_kmer[o] = x;
                s_val[o] = (bg << 30) | ((uint64_t)(code >> 1) << 2) | ((uint64_t)(code & 1u) << 1);
            }
            if (po < pos_cap) pos_keys[po] = ((uint64_t)c << 32) | (uint64_t)code;
            o++;
            po++;
        };
        for (int pos = threadIdx.x; pos < npos; pos += blockDim.x) {
            if (kmer_skipped(rs, re, nreg, pos, mt.K)) continue;
            const uint64_t fwd = packed_kmer(gb, pos, mt.K);
            const uint64_t rc = lm_revcomp(fwd, mt.K);
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const uint64_t x = s ? rc : fwd;
                const uint32_t pf = (uint32_t)(x >> shift);
                LM_PREFIX_MASKS(pf)
                for (int j = j0; j < j0 + nj; j++) {
                    if ((mt.masks[j] ^ x) != cap_min_load<LDS>(&hs[j])) continue;
                    if (x == 0 || lm_low_complexity(x, mt.K)) continue;
                    if (sweep == 0) mine++;
                    else emit(j, x, ((uint32_t)pos << 1) | (uint32_t)s);
                }
            }
        }
        // the captures of phase 1b (a k-mer reached here shares no prefix with its mask: the loop above never saw the pair)
        for (int r0 = 0; r0 < mt.M; r0 += blockDim.x) {
            const int j = r0 + threadIdx.x;
            const uint32_t first = j < mt.M ? mp[j] : 0u;
            const uint32_t cnt = first ? mc[j] : 0u;
            const unsigned long long mk = first ? mt.masks[j] : 0ull, hj = first ? cap_min_load<LDS>(&hs[j]) : 0ull;
            const uint64_t x = hj ^ mk;
            const bool act = first != 0 && x != 0 && !lm_low_complexity(x, mt.K);
            if (sweep == 0) {
                if (act) mine += cnt;
                continue;
            }
            if (act && cnt == 1) emit(j, x, first - 1u);
            const bool multi = act && cnt > 1;
            if (!__any(multi)) continue;
            for (int base = 0; base < npos; base += 64) { // every occurrence of a k-mer that occurs more than once
                const int pos = base + lane;
                const bool valid = pos < npos && !kmer_skipped(rs, re, nreg, pos, mt.K);
                uint64_t f = 0, r = 0;
                if (valid) {
                    f = packed_kmer(gb, pos, mt.K);
                    r = lm_revcomp(f, mt.K);
                }
                unsigned long long vm = __ballot(valid);
                while (vm) {
                    const int t = __builtin_amdgcn_readfirstlane(__ffsll((long long)vm) - 1);
                    vm &= vm - 1;
                    const uint64_t ff = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(f >> 32), t) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)f, t);
                    const uint64_t rr = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(r >> 32), t) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)r, t);
                    const uint32_t code = (uint32_t)(base + t) << 1;
                    if (multi && ff == x) emit(j, x, code);
                    if (multi && rr == x) emit(j, x, code | 1u);
                }
            }
        }
    }
    if (stamp) clk[3] = wall_clock64();
}

__global__ void k_pseudo_pos_g(GenomeTab gt, int64_t l0, int nchunk, int K, uint64_t *__restrict__ pos_keys, unsigned long long base) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < nchunk) pos_keys[base + c] = ((uint64_t)c << 32) | ((uint64_t)(uint32_t)(gt.g_len[l0 + c] - K) << 1) | 1ull; // sorts last
}

// Desert filling, lib-index-build.go:1094-1407, as the reference does it: for every pair of neighbouring seeds at least
// max_desert apart, walk from pre + seed_dist in steps of seed_dist; at each step scan seed_pos_r positions upstream, then
// downstream, for a non-low-complexity k-mer (+ strand before - strand) that IS THE CAPTURE OF SOME MASK WHEN THE WINDOW
// [pre - 1000, pos + 1000 + k) ALONE IS MASKED (MaskKnownDistinctPrefixes(window, nil, false), :1191-1240), and store it
// under that mask - the LAST (largest-index) mask that captures it.  A wavefront takes ppw (at most 64) seed pairs, finds the deserts
// among them and walks them one after the other; the capture test of a candidate is a sweep of the window by the 64 lanes
// (is any window k-mer of either strand with the same p-base prefix closer to the mask?).  The walk starts from pre = 0
// and ends at the pseudo position len - K of THAT record, the window is clipped to that record, and a candidate whose
// k-mer overlaps a skip region is passed over in the upstream and in the downstream scan (add_one's in_intervals) - the
// window masking itself ignores skip regions (MaskKnownDistinctPrefixes(window, nil, false), lib-index-build.go:1198).
__global__ __launch_bounds__(256) void k_desert_fill_g(GenomeTab gt, MaskTab mt, const uint8_t *__restrict__ gbits, int64_t l0,
                                                        const uint64_t *__restrict__ pos_keys, int64_t npk, int ppw, int max_desert,
                                                        int seed_dist, uint16_t *__restrict__ s_mask,
                                                        uint64_t *__restrict__ s_kmer, uint64_t *__restrict__ s_val,
                                                        unsigned long long *__restrict__ counter, unsigned long long cap) {
    const int seed_pos_r = seed_dist / 2;
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t base = wave * ppw; base < npk; base += nwaves * ppw) { // ppw (1 .. 64) seed pairs per wavefront
        const int64_t t = base + lane;
        int c = 0, pos = 0, pre = 0;
        bool isd = false;
        if (lane < ppw && t < npk) {
            const uint64_t key = pos_keys[t];
            c = (int)(key >> 32);
            pos = (int)((key & 0xffffffffu) >> 1);
            if (t > 0 && (int)(pos_keys[t - 1] >> 32) == c) pre = (int)((pos_keys[t - 1] & 0xffffffffu) >> 1);
            isd = pos - pre >= max_desert;
        }
        uint64_t todo = __ballot(isd);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int gc = __builtin_amdgcn_readfirstlane(__shfl(c, src, 64));
            const int gpos = __builtin_amdgcn_readfirstlane(__shfl(pos, src, 64));
            const int gpre = __builtin_amdgcn_readfirstlane(__shfl(pre, src, 64));
            const int64_t l = l0 + gc;
            const uint8_t *gb = gbits + gt.g_off[l];
            const int glen = gt.g_len[l];
            const uint64_t bg = gt.g_bg[l];
            const int32_t *rs = gt.reg_s + gt.reg_off[l], *re = gt.reg_e + gt.reg_off[l];
            const int nreg = gt.reg_off[l + 1] - gt.reg_off[l];
            int wstart = gpre - 1000;
            if (wstart < 0) wstart = 0;
            int wend = gpos + 1000 + mt.K;
            if (wend > glen) wend = glen;
            const int nk = wend - wstart - mt.K + 1; // k-mers of the window
            auto try_at = [&](int at, uint64_t *kmer, int *strand, int *im) { // the candidate at record position `at`
                const int rel = at - wstart;
                if (rel < 0 || rel >= nk) return false;
                if (kmer_skipped(rs, re, nreg, at, mt.K)) return false;
                const uint64_t f = packed_kmer(gb, at, mt.K);
                if (f != 0 && !lm_low_complexity(f, mt.K)) {
                    const int m = desert_capturing_mask(mt, gb, wstart, nk, f, lane);
                    if (m >= 0) {
                        *kmer = f;
                        *strand = 0;
                        *im = m;
                        return true;
                    }
                }
                const uint64_t r = lm_revcomp(f, mt.K);
                if (r != 0 && !lm_low_complexity(r, mt.K)) {
                    const int m = desert_capturing_mask(mt, gb, wstart, nk, r, lane);
                    if (m >= 0) {
                        *kmer = r;
                        *strand = 1;
                        *im = m;
                        return true;
                    }
                }
                return false;
            };
            int j = gpre + seed_dist;
            while (j < gpos) {
                const int start_dn = j + 1, end_up = j - seed_pos_r;
                bool ok = false;
                uint64_t kmer = 0;
                int strand = 0, im = -1, at = j;
                for (; at > end_up; at--)
                    if (try_at(at, &kmer, &strand, &im)) {
                        ok = true;
                        break;
                    }
                if (!ok) {
                    if (start_dn >= gpos) break;
                    int end_dn = start_dn + seed_pos_r;
                    if (end_dn >= gpos) end_dn = gpos - 1;
                    for (at = start_dn; at < end_dn; at++)
                        if (try_at(at, &kmer, &strand, &im)) {
                            ok = true;
                            break;
                        }
                }
                if (ok && lane == 0) {
                    const unsigned long long o = atomicAdd(counter, 1ull);
                    if (o < cap) {
                        s_mask[o] = (uint16_t)im;
                        s_kmer[o] = kmer;
                        s_val[o] = (bg << 30) | ((uint64_t)at << 2) | ((uint64_t)strand << 1);
                    }
                }
                j = at + seed_dist;
            }
        }
    }
}

} // namespace lm

struct lm_index_builder {
    lm_build_opt bo;
    lm_res_request rq;
    lm_index *ix = nullptr;
    std::string err;
    bool broken = false;              // a device error left a genome half added
    int64_t nrecords = 0, ninput = 0, input_bases = 0, max_len = 1;
    int nlists = 0;
    // the 2-bit store while it grows: device slabs laid out as consecutive pieces of the final store
    struct Slab {
        lm::DBuf<uint8_t> d;
        int64_t first = 0, used = 0, cap = 0;
    };
    std::vector<std::unique_ptr<Slab>> slabs;
    int64_t slab_bytes = (int64_t)256 << 20, store_bytes = 0;
    // lm_index_builder_extend: the index this builder continues (borrowed, only read) and its record count over all shards
    lm_index *base = nullptr;
    int64_t base_records = 0;
    // Resident indexes whose records this builder borrows (only read): the base, all of its local records under their own keys
    // (new_bg empty), then one entry per lm_index_builder_add_index.  recs: (local record there, local record here); the store
    // slots here are planned when the records are appended and filled by finish.  borrowed[l]: record l of ix->host.genomes
    // is one of them - its seeds are decoded from the source's image, not captured.
    struct Source {
        lm_index *ix = nullptr;
        std::vector<uint64_t> new_bg; // [the source's local records] key here or JOIN_DROP (lm_join_plan.h)
        bool drops = false;
        std::vector<std::pair<int64_t, int64_t>> recs;
    };
    std::vector<Source> sources;
    std::vector<uint8_t> borrowed;
    std::vector<int32_t> reg_off{0}, reg_s, reg_e; // skip regions of the local records (CSR)
    std::vector<int32_t> g2local;                  // sharded: record number -> local number or -1
    std::vector<int32_t> pfx;
    lm::PBuf<uint8_t> stage;
    lm::DBuf<uint8_t> d_ascii;
    lm::DBuf<int64_t> d_src;
    lm::DBuf<int32_t> d_dst, d_len;
    ~lm_index_builder() {
        if (ix) {
            (void)hipSetDevice(ix->device);
            if (ix->lane[0].main.st) (void)hipStreamSynchronize(ix->lane[0].main.st);
        }
        slabs.clear();
        if (ix) lm_index_close(ix);
    }
};

namespace lm {

// packs one record into the growing store (its slot: build_slot_bytes, zero-padded); returns its byte offset in the final store
static int64_t builder_pack(lm_index_builder *b, const BuildRecord &r, const lm_contig *contigs) {
    lm_index *ix = b->ix;
    const hipStream_t st = ix->lane[0].main.st;
    const int64_t slot = build_slot_bytes(r.len);
    if (b->slabs.empty() || b->slabs.back()->used + slot > b->slabs.back()->cap) {
        std::unique_ptr<lm_index_builder::Slab> s(new lm_index_builder::Slab());
        s->cap = std::max<int64_t>(b->slab_bytes, slot);
        s->first = b->store_bytes;
        s->d.alloc_exact((size_t)s->cap + 64, true, st);
        b->slabs.push_back(std::move(s));
    }
    lm_index_builder::Slab &sl = *b->slabs.back();
    std::vector<int64_t> src((size_t)r.n);
    std::vector<int32_t> len((size_t)r.n);
    int64_t total = 0;
    for (int c = 0; c < r.n; c++) {
        src[(size_t)c] = total;
        len[(size_t)c] = (int32_t)contigs[r.first + c].len;
        total += contigs[r.first + c].len;
    }
    // (the caller's memory may move after the call: everything is staged in pinned memory and on the device before it returns)
    b->stage.ensure((size_t)total + 64);
    for (int c = 0; c < r.n; c++)
        if (len[(size_t)c] > 0) memcpy(b->stage.p + src[(size_t)c], contigs[r.first + c].seq, (size_t)len[(size_t)c]);
    b->d_ascii.ensure((size_t)total + 64);
    b->d_src.ensure((size_t)r.n);
    b->d_dst.ensure((size_t)r.n);
    b->d_len.ensure((size_t)r.n);
    if (total > 0) HIPCHK(hipMemcpyAsync(b->d_ascii.p, b->stage.p, (size_t)total, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->d_src.p, src.data(), (size_t)r.n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->d_dst.p, r.dst_off.data(), (size_t)r.n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->d_len.p, len.data(), (size_t)r.n * 4, hipMemcpyHostToDevice, st));
    // (a slab is zeroed when it is cut, but a genome that failed half way may have been here before: the padding must be zero)
    HIPCHK(hipMemsetAsync(sl.d.p + sl.used, 0, (size_t)slot, st));
    hipLaunchKernelGGL(k_pack_record, dim3(gridn(((int64_t)r.len + 3) >> 2)), dim3(256), 0, st, b->d_ascii.p, b->d_src.p, b->d_dst.p,
                       b->d_len.p, r.n, r.len, sl.d.p + sl.used);
    HIPCHK(hipGetLastError());
    bsync(ix);
    const int64_t off = sl.first + sl.used;
    sl.used += slot;
    b->store_bytes = off + slot;
    return off;
}

// the host refused the pinned memory for the records beyond the residency budget: LM_ERR_NOMEM in every front end
struct PinnedOOM : DeviceOOM {
    using DeviceOOM::DeviceOOM;
};

// The settings of the seed pipeline, checked once for all front ends; false: `err` says what is wrong (LM_ERR_ARG).
// Only the GENERATED masks are limited to k = 31 and 2 * 4^p masks: gen_masks puts every p-base prefix once and the rest on
// distinct prefixes.  A set that is given - by the caller (lm_index_builder_new_masks) or by the resident index that is
// continued - may have any k and shape lm_mask_plan.h accepts; builder_header checks it.  A desert walk advances by seed_dist.
static bool seed_settings_ok(const char *who, int k, int masks, int max_desert, int seed_dist, bool generated, std::string &err) {
    if (!generated) {
        if (k < MASK_PLAN_MIN_K || k > MASK_PLAN_MAX_K || masks < MASK_PLAN_MIN_MASKS || masks > MASK_PLAN_MAX_MASKS || max_desert < 1 || seed_dist < 1) {
            err = std::string(who) + ": unsupported settings (k = " + std::to_string(k) + " must be in [10, 32], the number of masks = " + std::to_string(masks) +
                  " in [4, 65535], max_desert and seed_dist >= 1)";
            return false;
        }
        return true;
    }
    if (k != 31 || masks < 4 || masks > 65535 || max_desert < 1 || seed_dist < 1) {
        err = std::string(who) + ": unsupported settings (k must be 31, masks in [4, 65535], max_desert and seed_dist >= 1; only the generated masks "
              "are limited to k = 31: lm_index_builder_new_masks takes the caller's masks with k in [10, 32])";
        return false;
    }
    const int p = mask_prefix_of(masks);
    if (masks > 2 * (1 << (2 * p))) {
        err = std::string(who) + ": " + std::to_string(masks) + " masks need more than two masks per " + std::to_string(p) +
              "-base prefix, which the mask generator of this build does not make (at most " + std::to_string(2 * (1 << (2 * p))) +
              "; only the generated masks are limited: lm_index_builder_new_masks takes up to 32 masks on a prefix)";
        return false;
    }
    return true;
}
static bool build_opt_ok(const char *who, const lm_build_opt &bo, bool generated, std::string &err) {
    if (!seed_settings_ok(who, bo.k, bo.masks, bo.max_desert, bo.seed_dist, generated, err)) return false;
    if (bo.genome_batch_size < 1 || bo.genome_batch_size > (1 << 17) || bo.contig_interval < 0 || bo.contig_interval >= (1 << 28) ||
        bo.max_genome >= (1 << 28)) {
        err = std::string(who) + ": unsupported build options (genome_batch_size in [1, 2^17], contig_interval >= 0, max_genome < 2^28)";
        return false;
    }
    return true;
}

// What every front end begins with, ix->opt and ix->device being set: the stream, the HostIndex header, the mask set
// (generated, the caller's `given`, or the masks of the index `bh` that is continued), checked by the one rule of
// lm_mask_plan.h, pfx[f] = first mask of the p-base prefix f, and the upload of both.  `who`: the entry point, for the text.
// LM_OK, or the status to return with its text in g_open_error.
static lm_status builder_header(const char *who, lm_index *ix, int K, int M, int64_t mask_seed, int contig_interval, const HostIndex *bh,
                                const uint64_t *given, std::vector<int32_t> &pfx) {
    HostIndex &h = ix->host;
    // (the masks first: a set that is refused costs no device work)
    if (bh) h.masks = bh->masks;
    else if (given) h.masks.assign(given, given + M);
    else gen_masks(K, M, (uint64_t)mask_seed, h.masks);
    MaskPlan mp;
    {
        std::string why;
        if (!plan_masks(K, h.masks.data(), h.masks.size(), mp, why)) {
            g_open_error = std::string(who) + ": the mask set cannot be built with: " + why;
            return LM_ERR_ARG;
        }
    }
    if (bh && bh->mask_prefix != mp.p) {
        g_open_error = std::string(who) + ": the index carries a mask prefix of " + std::to_string(bh->mask_prefix) + " bases, its " + std::to_string(M) +
                       " masks give " + std::to_string(mp.p);
        return LM_ERR_ARG;
    }
    HIPCHK(hipSetDevice(ix->device));
    HIPCHK(hipStreamCreate(&ix->lane[0].main.st));
    const lm_options &opt = ix->opt;
    const int p = mp.p;
    h.k = K;
    h.M = M;
    h.main_version = 3;
    h.minor_version = 5;
    h.synthetic = false;
    h.mask_prefix = p;
    h.anchor_prefix = bh ? bh->anchor_prefix : 6;
    h.contig_interval = contig_interval;
    h.shard_rank = bh ? bh->shard_rank : opt.shard_count > 1 ? opt.shard_rank : 0;
    h.shard_count = bh ? bh->shard_count : opt.shard_count > 1 ? opt.shard_count : 1;
    if (h.shard_rank < 0 || h.shard_rank >= h.shard_count) {
        g_open_error = "index build: shard_rank outside [0, shard_count)";
        return LM_ERR_OPTION;
    }
    if (!bh && (opt.min_prefix > K || opt.min_prefix < p + h.anchor_prefix)) { // (a base's options passed when it was made)
        g_open_error = "MinPrefix out of range for this index";
        return LM_ERR_OPTION;
    }
    pfx = std::move(mp.pfx_first);
    ix->d_masks.ensure((size_t)M);
    ix->d_pfx_first.ensure(pfx.size());
    HIPCHK(hipMemcpyAsync(ix->d_masks.p, h.masks.data(), (size_t)M * 8, hipMemcpyHostToDevice, ix->lane[0].main.st));
    HIPCHK(hipMemcpyAsync(ix->d_pfx_first.p, pfx.data(), pfx.size() * 4, hipMemcpyHostToDevice, ix->lane[0].main.st));
    bsync(ix);
    return LM_OK;
}

// How k_capture_g finds the masks of a prefix and where it keeps the minima, for a set of M masks with the prefix table pfx
// (4^p + 1 entries): one decision for the builder and for genome screening.
struct CapturePlan {
    bool csr = false, lds_capture = false, tab_lds = false;
    size_t lds_bytes = 0;
    std::vector<uint64_t> dmap; // doubled-prefix map and per-word counts (CSR = false)
    std::vector<uint32_t> dcnt;
};
static CapturePlan capture_plan(int M, int p, const std::vector<int32_t> &pfx) {
    CapturePlan c;
    const int npfx = 1 << (2 * p), nwords = (npfx + 63) >> 6;
    std::vector<uint64_t> &dmap = c.dmap;
    std::vector<uint32_t> &dcnt = c.dcnt;
    dmap.assign((size_t)nwords, 0);
    dcnt.assign((size_t)nwords, 0);
    bool csr = false;
    for (int f = 0; f < npfx; f++) {
        const int n = pfx[(size_t)f + 1] - pfx[(size_t)f];
        if (n == 2) dmap[(size_t)(f >> 6)] |= 1ull << (f & 63);
        if (n < 1 || n > 2) csr = true;
    }
    for (int w = 1; w < nwords; w++) dcnt[(size_t)w] = dcnt[(size_t)w - 1] + (uint32_t)__builtin_popcountll(dmap[(size_t)w - 1]);
    // capture in LDS when the per-mask minima fit a CU's LDS, otherwise minima in a global table (one threshold for both ways
    // to find the masks of a prefix).  The prefix table of the CSR instantiations is staged in LDS where it fits beside them:
    // always for p <= 6 (16 KB at most, under 16384 x 8 B of minima) and for p = 7 with the minima in a global table (64 KB on
    // its own); with p = 7 and the minima in LDS (16384 .. ~20000 masks: 128 .. 160 KB) it cannot, and is read from global
    // memory.  LM_BUILD_PFX_GLOBAL (measurement only; results do not depend on it) keeps it there always.
    const size_t lds_full = (size_t)M * 8 + (size_t)nwords * 12 + 64;
    const bool lds_capture = lds_full <= 160 * 1024;
    const size_t csr_base = (lds_capture ? (size_t)M * 8 : 0) + 64, csr_tab = ((size_t)npfx + 1) * 4;
    const bool tab_lds = csr && csr_base + csr_tab + 16 <= 160 * 1024 && getenv("LM_BUILD_PFX_GLOBAL") == nullptr;
    const size_t lds_bytes = csr ? csr_base + (tab_lds ? csr_tab : 0) : lds_capture ? lds_full : (size_t)nwords * 12 + 64;
    c.csr = csr;
    c.lds_capture = lds_capture;
    c.tab_lds = tab_lds;
    c.lds_bytes = lds_bytes;
    return c;
}
template <bool KM> static decltype(&k_capture_g<true, false, false, KM>) capture_kernel(const CapturePlan &c) {
    return !c.csr ? (c.lds_capture ? k_capture_g<true, false, false, KM> : k_capture_g<false, false, false, KM>)
           : c.lds_capture ? (c.tab_lds ? k_capture_g<true, true, true, KM> : k_capture_g<true, true, false, KM>)
                           : (c.tab_lds ? k_capture_g<false, true, true, KM> : k_capture_g<false, true, false, KM>);
}

// The seed pipeline, what every front end ends in.  In: the header and `pfx` of builder_header; the 2-bit store ix->d_gbits
// with the records in slots of build_slot_bytes back to back, described by h.genomes (bits_off, len, bg); h.batch_first;
// h.g2local where the records of a sharded set are numbered through a table.  It uploads the tables, fills in the view,
// generates the seeds and applies the residency request `rq`.
// Seeds are generated per chunk of records into staging arrays and shown to the packer, twice (count, place): the unpacked
// seeds of the whole set never exist (they would not fit beside the packed image at BASELINE configs 3-5).  A chunk holds
// at most chunk_records records and chunk_bases bases - the caller's choice: a record of a chunk costs 16 B x masks of
// scratch (24 B with the minima in a global table), a chunk one host synchronisation per phase.
// reg_off / reg_s / reg_e: CSR of the skip regions of every record (all zeros: none).  The record list is a sequence of runs
// that are either captured or borrowed from a resident index (borrowed[l] != 0; empty: every record is captured): the seeds
// of a borrowed record are decoded from the image of its source - `sources`, in the order their records come - and given
// the record's key here (SeedSource::new_bg; null: the source's own keys, the base of lm_index_builder_extend).  Capture
// chunks are cut from captured runs only, and a borrowed record has no skip regions.
struct SeedSource {
    const lm_index *ix;
    const std::vector<uint64_t> *new_bg; // null or [ix's local records]: lm_join_plan.h
    bool drops;                          // some entry is JOIN_DROP: the decode compacts
    const char *what;                    // LM_DEBUG: "the base" / "source N"
};
static void build_seed_index(lm_index *ix, const std::vector<int32_t> &pfx, const std::vector<int32_t> &reg_off, const std::vector<int32_t> &reg_s,
                             const std::vector<int32_t> &reg_e, int max_desert, int seed_dist, int64_t chunk_records, int64_t chunk_bases,
                             const std::vector<SeedSource> &sources, const std::vector<uint8_t> &borrowed, const lm_res_request &rq) {
    HostIndex &h = ix->host;
    const hipStream_t st = ix->lane[0].main.st;
    const int K = h.k, M = h.M, p = h.mask_prefix;
    const int64_t nlocal = (int64_t)h.genomes.size();
    const bool dbg = getenv("LM_DEBUG") != nullptr;
    const double t0 = now_ms();
    // measurement / tests only, results do not depend on it: a first size of the staging arrays that
    // overflows, and (the base's seeds may be decoded in pieces smaller than what a capture needs) the largest decode piece
    int64_t stage_seeds = 0, piece_seeds = 0;
    if (const char *e = getenv("LM_BUILD_STAGE_SEEDS")) {
        stage_seeds = std::max<int64_t>(1024, atoll(e));
        piece_seeds = std::max<int64_t>(4, atoll(e));
    }
    auto copy_up = [&](auto &dbuf, const auto &vec) {
        dbuf.ensure(std::max<size_t>(vec.size(), 1));
        if (!vec.empty()) HIPCHK(hipMemcpyAsync(dbuf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, st));
    };
    // ---- tables
    std::vector<int64_t> goff((size_t)nlocal), slot((size_t)nlocal);
    std::vector<int32_t> glen((size_t)nlocal);
    std::vector<uint64_t> gbg((size_t)nlocal);
    int64_t max_len = 1;
    for (int64_t l = 0; l < nlocal; l++) {
        const HostGenome &G = h.genomes[(size_t)l];
        goff[(size_t)l] = G.bits_off;
        glen[(size_t)l] = G.len;
        gbg[(size_t)l] = G.bg;
        slot[(size_t)l] = build_slot_bytes(G.len);
        max_len = std::max<int64_t>(max_len, G.len);
        ix->bg2local[G.bg] = (int)l;
    }
    const int64_t store_bytes = nlocal ? goff.back() + slot.back() : 0;
    copy_up(ix->d_g_off, goff);
    copy_up(ix->d_g_len, glen);
    copy_up(ix->d_g_bg, gbg);
    copy_up(ix->d_batch_first, h.batch_first);
    if (!h.g2local.empty()) copy_up(ix->d_g2local, h.g2local);
    DBuf<int32_t> d_reg_off, d_reg_s, d_reg_e;
    copy_up(d_reg_off, reg_off);
    copy_up(d_reg_s, reg_s);
    copy_up(d_reg_e, reg_e);
    lm_fill_gap_lut(ix); // same table as lm_index_open (lib-chaining.go:662-667)
    bsync(ix);
    DevIndexView &v = ix->view;
    v.K = K;
    v.M = M;
    v.mask_prefix = p;
    v.masks = ix->d_masks.p;
    v.pfx_first = ix->d_pfx_first.p;
    v.g_bg = ix->d_g_bg.p;
    v.gbits = ix->d_gbits.p;
    v.g_off = ix->d_g_off.p;
    v.g_len = ix->d_g_len.p;
    v.batch_first = ix->d_batch_first.p;
    v.nbatches = h.genome_batches;
    v.ngenomes = nlocal;
    v.shard_rank = h.shard_rank;
    v.shard_count = h.shard_count;
    v.g2local = h.g2local.empty() ? nullptr : ix->d_g2local.p;
    const MaskTab mt{ix->d_masks.p, ix->d_pfx_first.p, K, p, M};
    const GenomeTab gt{ix->d_g_off.p, ix->d_g_len.p, ix->d_g_bg.p, d_reg_off.p, d_reg_s.p, d_reg_e.p};
    // ---- prefix -> masks (k_capture_g).  Every prefix once or twice (every generated set, and a caller's set of that shape):
    // without a table in memory, from the doubled-prefix map.  Otherwise (builder_header checked the set: up to 32 masks on a
    // prefix) from the prefix table the handle carries, ix->d_pfx_first.
    const CapturePlan cp = capture_plan(M, p, pfx);
    const bool csr = cp.csr, lds_capture = cp.lds_capture, tab_lds = cp.tab_lds;
    const size_t lds_bytes = cp.lds_bytes;
    DBuf<uint64_t> dbl_map;
    DBuf<uint32_t> dbl_cnt;
    copy_up(dbl_map, cp.dmap);
    copy_up(dbl_cnt, cp.dcnt);
    using CaptureKernel = decltype(&k_capture_g<true, false, false>);
    const CaptureKernel capture = capture_kernel<false>(cp);
    if (lds_bytes > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)capture, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    if (dbg)
        fprintf(stderr, "[lm] builder: capture with the minima in %s, the masks of a prefix from %s\n", lds_capture ? "LDS" : "a global table",
                !csr ? "the doubled-prefix map" : tab_lds ? "the prefix table in LDS" : "the prefix table in global memory");
    // ---- chunks of records within the caller's limits (and 192 MB of minima where they live in a global table); the staging
    // arrays are sized from the largest chunk with one estimate per record
    const int64_t ch_max = std::max<int64_t>(1, lds_capture ? chunk_records : std::min<int64_t>(chunk_records, ((int64_t)192 << 20) / ((int64_t)M * 8)));
    struct Chunk {
        int64_t l0;
        int n;
        double seeds, pos;
    };
    std::vector<Chunk> chunks; // (of the captured records only: a chunk never reaches across a borrowed run)
    auto is_borrowed = [&](int64_t l) { return !borrowed.empty() && borrowed[(size_t)l] != 0; };
    for (int64_t l = 0; l < nlocal;) {
        if (is_borrowed(l)) {
            l++;
            continue;
        }
        Chunk c{l, 0, 0, 0};
        int64_t bases = 0;
        while (l < nlocal && !is_borrowed(l) && c.n < ch_max && (c.n == 0 || bases + glen[(size_t)l] <= chunk_bases)) {
            bases += glen[(size_t)l];
            c.seeds += 2.0 * (1.45 * M + (double)glen[(size_t)l] / 42.0) + 1024;
            c.pos += 1.45 * M + 64;
            c.n++;
            l++;
        }
        chunks.push_back(c);
    }
    int ch_n = 1;
    double est_seeds = 0, est_pos = 0;
    for (auto &c : chunks) {
        ch_n = std::max(ch_n, c.n);
        est_seeds = std::max(est_seeds, c.seeds);
        est_pos = std::max(est_pos, c.pos);
    }
    unsigned long long cap = (unsigned long long)est_seeds + 65536, pos_cap = (unsigned long long)est_pos + (unsigned long long)ch_n + 64;
    // the sources' seeds pass through the same arrays in pieces: large enough that a big image is not cut into thousands of launches
    struct SrcTabs {
        std::vector<int64_t> md_off, out_off;
        int64_t n_main = 0, n_out = 0;
        DBuf<uint64_t> new_bg;
    };
    std::vector<std::unique_ptr<SrcTabs>> stabs;
    for (const SeedSource &S : sources) {
        std::unique_ptr<SrcTabs> t(new SrcTabs());
        t->md_off.resize((size_t)2 * M + 1);
        t->out_off.resize((size_t)2 * M + 1);
        HIPCHK(hipMemcpyAsync(t->md_off.data(), S.ix->d_md_off.p, t->md_off.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(t->out_off.data(), S.ix->d_out_off.p, t->out_off.size() * 8, hipMemcpyDeviceToHost, st));
        if (S.new_bg) {
            if ((int64_t)S.new_bg->size() != S.ix->view.ngenomes) throw HipError("index build: a source's key table does not match its records");
            copy_up(t->new_bg, *S.new_bg);
        }
        bsync(ix);
        t->n_main = t->md_off.back();
        t->n_out = t->out_off.back();
        cap = std::max<unsigned long long>(cap, (unsigned long long)std::min<int64_t>(std::max(t->n_main, t->n_out), (int64_t)1 << 26));
        stabs.push_back(std::move(t));
    }
    if (stage_seeds > 0) { // (tests: a first estimate that is too small, so that the enlarge-and-retry path runs)
        cap = (unsigned long long)stage_seeds;
        pos_cap = (unsigned long long)stage_seeds + (unsigned long long)ch_n + 64;
    }
    DBuf<uint16_t> s_mask;
    DBuf<uint64_t> s_kmer, s_val, pos_keys, pos_keys2;
    auto size_staging = [&]() {
        s_mask.alloc_exact(cap);
        s_kmer.alloc_exact(cap);
        s_val.alloc_exact(cap);
        pos_keys.alloc_exact(pos_cap);
        pos_keys2.alloc_exact(pos_cap);
    };
    size_staging();
    DBuf<unsigned long long> counters, hashes;
    counters.ensure(8);
    hashes.alloc_exact(lds_capture ? 1 : (size_t)ch_n * M);
    DBuf<uint32_t> miss_pos, miss_cnt;
    miss_pos.alloc_exact((size_t)ch_n * M);
    miss_cnt.alloc_exact((size_t)ch_n * M);
    SeedPacker packer;
    packer.begin(ix, nlocal, max_len);
    double t_cap = 0, t_desert = 0, t_pack = 0;
    // the seeds of one chunk in the staging arrays; false: an array was too small - `cap` / `pos_cap` are what it takes
    // (nothing was written past an array: every store is guarded by its capacity)
    auto generate = [&](const Chunk &c, unsigned long long &nseeds) {
        const unsigned long long pos_lim = pos_cap - (unsigned long long)c.n - 1;
        const double ta = now_ms();
        HIPCHK(hipMemsetAsync(counters.p, 0, 2 * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(capture, dim3(c.n), dim3(1024), lds_bytes, st, gt, mt, ix->d_gbits.p, c.l0, dbl_map.p, dbl_cnt.p, hashes.p,
                           miss_pos.p, miss_cnt.p, s_mask.p, s_kmer.p, s_val.p, counters.p, cap, pos_keys.p, counters.p + 1, pos_lim,
                           dbg ? (unsigned long long *)(counters.p + 4) : nullptr);
        HIPCHK(hipGetLastError());
        unsigned long long hc[8];
        HIPCHK(hipMemcpyAsync(hc, counters.p, sizeof hc, hipMemcpyDeviceToHost, st));
        bsync(ix);
        const double tb = now_ms();
        t_cap += tb - ta;
        if (dbg)
            fprintf(stderr, "[lm] builder: capture of record %lld (%d bases): argmin %.3f ms, missing-prefix pass %.3f ms, emit %.3f ms\n",
                    (long long)c.l0, glen[(size_t)c.l0], (double)(hc[5] - hc[4]) * 1e-5, (double)(hc[6] - hc[5]) * 1e-5, (double)(hc[7] - hc[6]) * 1e-5);
        if (hc[0] >= cap || hc[1] >= pos_lim) {
            // (desert and reversed seeds come on top of the captures: about as many again, twice over)
            cap = std::max(cap, hc[0] * 4 + 65536);
            pos_cap = std::max(pos_cap, hc[1] * 2 + (unsigned long long)ch_n + 64);
            return false;
        }
        unsigned long long npk = hc[1];
        hipLaunchKernelGGL(k_pseudo_pos_g, dim3((c.n + 63) / 64), dim3(64), 0, st, gt, c.l0, c.n, K, pos_keys.p, npk);
        npk += (unsigned long long)c.n;
        prim_sort_keys(st, ix->lane[0].main.tmp, pos_keys.p, pos_keys2.p, (size_t)npk, 0, 64);
        // A wavefront walks the deserts among its seed pairs one after the other.  64 pairs each where there are pairs enough to
        // fill the device that way (any set of the usual mask counts); fewer where there are not - a record set under a few dozen
        // masks has a few hundred pairs, nearly all of them deserts of thousands of bases whose every candidate fails its window
        // sweep, and five wavefronts walking 64 of those each take a minute where one wavefront per desert takes a second
        const int ppw = (int)std::max<int64_t>(1, std::min<int64_t>(64, (int64_t)npk / 8192));
        hipLaunchKernelGGL(k_desert_fill_g, dim3(gridn(((int64_t)npk + ppw - 1) / ppw, 4)), dim3(256), 0, st, gt, mt, ix->d_gbits.p, c.l0,
                           pos_keys2.p, (int64_t)npk, ppw, max_desert, seed_dist, s_mask.p, s_kmer.p, s_val.p, counters.p, cap);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hc, counters.p, sizeof hc, hipMemcpyDeviceToHost, st));
        bsync(ix);
        if (hc[0] >= cap) {
            cap = hc[0] * 3 + 65536;
            return false;
        }
        const unsigned long long upto = hc[0];
        hipLaunchKernelGGL(k_reverse_seeds, dim3(gridn((int64_t)upto)), dim3(256), 0, st, mt, 0ull, upto, s_mask.p, s_kmer.p, s_val.p,
                           counters.p, cap);
        HIPCHK(hipMemcpyAsync(hc, counters.p, sizeof hc, hipMemcpyDeviceToHost, st));
        bsync(ix);
        if (hc[0] >= cap) {
            cap = hc[0] + hc[0] / 4 + 65536;
            return false;
        }
        nseeds = hc[0];
        t_desert += now_ms() - tb;
        return true;
    };
    double t_base = 0, t_dump = 0;
    for (int pass = 0; pass < 2; pass++) {
        for (size_t si = 0; si < sources.size(); si++) {
            // a source's seeds, decoded in pieces no larger than the staging arrays (a list longer than a piece is cut); every
            // value is re-encoded by the packer: gid_bits / pos_bits of the new set may be wider than the source's.  Where the
            // source keeps only some of its records the kernel compacts and the host reads the piece's count (8 bytes): a
            // piece may come out empty
            const SeedSource &S = sources[si];
            SrcTabs &T = *stabs[si];
            const uint64_t *nbg = S.new_bg ? T.new_bg.p : nullptr;
            unsigned long long *n_out = S.drops ? counters.p + 2 : nullptr;
            const double tb0 = now_ms();
            const int64_t piece = piece_seeds > 0 ? std::min<int64_t>(piece_seeds, (int64_t)cap) : (int64_t)cap;
            int64_t kept_seeds = 0;
            for (int flat = 0; flat < 2; flat++) {
                const int64_t total = flat ? T.n_out : T.n_main;
                for (int64_t s0 = 0; s0 < total; s0 += piece) {
                    int64_t n = std::min<int64_t>(piece, total - s0);
                    const double td0 = dbg ? (bsync(ix), now_ms()) : 0;
                    if (n_out) HIPCHK(hipMemsetAsync(n_out, 0, sizeof(unsigned long long), st));
                    sp_dump_range(S.ix, st, flat ? T.out_off : T.md_off, flat != 0, s0, s0 + n, s_mask.p, s_kmer.p, s_val.p, nbg, n_out);
                    if (n_out) {
                        unsigned long long got = 0;
                        HIPCHK(hipMemcpyAsync(&got, n_out, sizeof got, hipMemcpyDeviceToHost, st));
                        bsync(ix);
                        if (got > (unsigned long long)n) throw HipError("index build: a compacted decode piece holds more seeds than were decoded");
                        n = (int64_t)got;
                    }
                    if (dbg) {
                        bsync(ix);
                        t_dump += now_ms() - td0;
                    }
                    kept_seeds += n;
                    if (pass == 0) packer.count(s_mask.p, s_kmer.p, s_val.p, n);
                    else packer.place(s_mask.p, s_kmer.p, s_val.p, n);
                }
            }
            bsync(ix);
            t_base += now_ms() - tb0;
            if (dbg)
                fprintf(stderr, "[lm] builder pass %d: %s's %lld seeds (%lld outliers; %lld kept, %s) decoded and packed in pieces of %lld: %.1f ms, "
                                "of which the decode kernel %.1f ms (cumulative)\n", pass, S.what, (long long)(T.n_main + T.n_out), (long long)T.n_out,
                        (long long)kept_seeds, !S.new_bg ? "keys as they are" : S.drops ? "keys rewritten, compacted" : "keys rewritten",
                        (long long)piece, t_base, t_dump);
        }
        for (const Chunk &c : chunks) {
            unsigned long long n = 0;
            for (int attempt = 0; !generate(c, n); attempt++) {
                // a record set that outgrows the estimate (a k-mer repeated thousands of times under many masks) takes a larger try
                if (attempt >= 4) throw HipError("index build: the seed staging buffers outgrew four enlargements");
                if (dbg) fprintf(stderr, "[lm] builder: staging buffers enlarged to %llu seeds / %llu positions\n", cap, pos_cap);
                size_staging();
            }
            const double tc = now_ms();
            if (pass == 0) packer.count(s_mask.p, s_kmer.p, s_val.p, (int64_t)n);
            else packer.place(s_mask.p, s_kmer.p, s_val.p, (int64_t)n);
            bsync(ix);
            t_pack += now_ms() - tc;
        }
        if (pass == 0) packer.end_count();
        if (dbg)
            fprintf(stderr, "[lm] builder pass %d: capture %.1f ms, desert+reverse %.1f ms, packer %.1f ms (cumulative)\n", pass, t_cap,
                    t_desert, t_pack);
    }
    hashes.release();
    miss_pos.release();
    miss_cnt.release();
    pos_keys.release();
    pos_keys2.release();
    s_mask.release();
    s_kmer.release();
    s_val.release();
    const double tf = now_ms();
    packer.finish();
    if (dbg)
        fprintf(stderr, "[lm] builder: partition sort %.1f ms; %lld records, %lld seeds (%lld outliers), %.2f B/seed; seed pipeline %.1f ms\n",
                now_ms() - tf, (long long)nlocal, (long long)ix->n_seeds, (long long)ix->n_seeds_outlier,
                (double)ix->seed_bytes / std::max<double>(1.0, (double)ix->n_seeds), now_ms() - t0);
    ix->lane[0].main.tmp.release();
    // ---- residency: the set is built in HBM as ever; the records beyond the budget then move to pinned host memory and the
    // device store shrinks to the rest (a set that does not fit the device DURING the build is out of reach of this form)
    ix->res.genomes_device = nlocal;
    ix->res.genome_bytes_device = store_bytes;
    {
        int64_t budget = rq.budget;
        if (rq.mode == LM_GENOMES_AUTO && budget == 0) {
            size_t fr = 0, tot = 0;
            HIPCHK(hipMemGetInfo(&fr, &tot));
            budget = lm_res_auto_budget((int64_t)fr + store_bytes, 0); // (the store itself is part of what it may take)
        }
        // the budget is counted in the store's slots: the first `keep` records stay, the rest go to the host - the planner
        // lays out the host side only
        int64_t keep = rq.mode == LM_GENOMES_HOST ? 0 : nlocal;
        if (rq.mode == LM_GENOMES_AUTO)
            for (keep = 0; keep < nlocal && goff[(size_t)keep] + slot[(size_t)keep] <= budget;) keep++;
        if (keep < nlocal) {
            const int64_t kept_bytes = keep > 0 ? goff[(size_t)keep - 1] + slot[(size_t)keep - 1] : 0;
            std::vector<int64_t> nbs;
            for (int64_t l = keep; l < nlocal; l++) nbs.push_back(((int64_t)glen[(size_t)l] + 3) >> 2);
            ResidencyPlan plan = plan_residency(nbs, LM_GENOMES_HOST, 0, LM_RES_SEGMENT_BYTES);
            plan.place.insert(plan.place.begin(), (size_t)keep, GenomePlace()); // (the kept records: in the device store)
            plan.genomes_device = keep;
            plan.bytes_device = kept_bytes;
            std::string e;
            if (!lm_res_alloc_host(ix, plan, e)) throw PinnedOOM(e);
            for (int64_t l = keep; l < nlocal; l++) { // (pinned destination: DMA at the link's rate, one copy per record)
                const GenomePlace &pl = plan.place[(size_t)l];
                HIPCHK(hipMemcpyAsync(ix->g_host_segs[(size_t)pl.seg].p + pl.off, ix->d_gbits.p + goff[(size_t)l], (size_t)nbs[(size_t)(l - keep)],
                                      hipMemcpyDeviceToHost, st));
                h.genomes[(size_t)l].bits_off = -1; // (not in the device store)
                goff[(size_t)l] = -1;
            }
            bsync(ix);
            {   // the device store shrinks to the records that stay (same offsets: they are its first bytes)
                DBuf<uint8_t> kept;
                kept.alloc_exact((size_t)kept_bytes + 64, true, st);
                if (kept_bytes > 0) HIPCHK(hipMemcpyAsync(kept.p, ix->d_gbits.p, (size_t)kept_bytes, hipMemcpyDeviceToDevice, st));
                bsync(ix);
                ix->d_gbits.release();
                std::swap(ix->d_gbits.p, kept.p);
                std::swap(ix->d_gbits.cap, kept.cap);
            }
            copy_up(ix->d_g_off, goff);
            bsync(ix);
            ix->view.gbits = ix->d_gbits.p;
        }
    }
    ix->hbm_bytes = ix->seed_bytes + (int64_t)((uint64_t)ix->res.genome_bytes_device + 64 + (uint64_t)M * 8 + pfx.size() * 4 + (uint64_t)nlocal * 20 +
                                               h.batch_first.size() * 8);
    lm_set_scratch_budget(ix);
}

// The genome front end's finish: the slabs (and the base's records) into one store, the host metadata lm_index_save writes,
// then the seed pipeline
static void builder_finish(lm_index_builder *b) {
    lm_index *ix = b->ix;
    const hipStream_t st = ix->lane[0].main.st;
    HostIndex &h = ix->host;
    const lm_build_opt &bo = b->bo;
    // ---- the store: one allocation, the slabs copied to their places (they ARE consecutive pieces of it) and released
    b->d_ascii.release();
    ix->d_gbits.alloc_exact((size_t)b->store_bytes + 64, true, st);
    for (auto &s : b->slabs)
        if (s->used > 0) HIPCHK(hipMemcpyAsync(ix->d_gbits.p + s->first, s->d.p, (size_t)s->used, hipMemcpyDeviceToDevice, st));
    bsync(ix);
    b->slabs.clear();
    const lm_index *base = b->base;
    for (const lm_index_builder::Source &S : b->sources) {
        // a source's records into the slots planned for them, record by record: an opened index packs its store more tightly
        // than build_slot_bytes, and a host-resident record comes from its pinned segment.  Device records whose slots lie as
        // far apart here as there (a source built by this builder, taken whole) go as one copy.
        const lm_index *src = S.ix;
        int64_t run_src = -1, run_dst = 0, run_len = 0;
        auto flush = [&]() {
            if (run_src >= 0) HIPCHK(hipMemcpyAsync(ix->d_gbits.p + run_dst, src->d_gbits.p + run_src, (size_t)run_len, hipMemcpyDeviceToDevice, st));
            run_src = -1;
        };
        for (const auto &sd : S.recs) {
            const HostGenome &G = h.genomes[(size_t)sd.second];
            const int64_t nb = ((int64_t)G.len + 3) >> 2, so = src->host.genomes[(size_t)sd.first].bits_off;
            const uint8_t *hp = src->g_hhost.empty() ? nullptr : src->g_hhost[(size_t)sd.first];
            if (hp) {
                flush();
                HIPCHK(hipMemcpyAsync(ix->d_gbits.p + G.bits_off, hp, (size_t)nb, hipMemcpyHostToDevice, st));
                continue;
            }
            if (run_src >= 0 && so - run_src == G.bits_off - run_dst && so >= run_src + run_len) {
                run_len = so - run_src + nb;
                continue;
            }
            flush();
            run_src = so;
            run_dst = G.bits_off;
            run_len = nb;
        }
        flush();
        bsync(ix);
    }
    // ---- host metadata
    h.total_bases = ix->opt.total_bases_override > 0 ? ix->opt.total_bases_override : b->input_bases;
    h.input_genomes = b->ninput;
    h.genome_batch_size = bo.genome_batch_size;
    if (!base) { // (a continued set keeps the settings it was begun with: _extend copied them from the base)
        h.rand_seed = bo.mask_seed;
        h.max_seed_dist = bo.max_desert;
        h.seed_dist_in_desert = bo.seed_dist;
    }
    h.genome_batches = (int)((b->nrecords + bo.genome_batch_size - 1) / bo.genome_batch_size);
    h.batch_first.assign((size_t)h.genome_batches + 1, 0);
    for (int i = 0; i <= h.genome_batches; i++) h.batch_first[(size_t)i] = std::min<int64_t>((int64_t)i * bo.genome_batch_size, b->nrecords);
    h.n_local_genomes = (int64_t)h.genomes.size();
    h.max_genome_len = b->max_len;
    h.has_chunks = !h.chunk_of.empty();
    if (h.shard_count > 1) h.g2local = b->g2local;
    // chunks of records: as many as the per-record scratch (16 B per mask) allows in 128 MB, and at most 2^30 bases
    const int64_t ch_records = std::min<int64_t>(2048, ((int64_t)128 << 20) / ((int64_t)h.M * 16));
    std::vector<SeedSource> sources;
    std::vector<std::string> names;
    for (size_t i = 0; i < b->sources.size(); i++) names.push_back(b->sources[i].ix == base ? std::string("the base") : "source " + std::to_string(i));
    for (size_t i = 0; i < b->sources.size(); i++) {
        const lm_index_builder::Source &S = b->sources[i];
        sources.push_back(SeedSource{S.ix, S.new_bg.empty() ? nullptr : &S.new_bg, S.drops, names[i].c_str()});
    }
    build_seed_index(ix, b->pfx, b->reg_off, b->reg_s, b->reg_e, bo.max_desert, bo.seed_dist, ch_records, (int64_t)1 << 30, sources, b->borrowed, b->rq);
}

} // namespace lm

extern "C" {

void lm_build_opt_default(lm_build_opt *o) {
    if (!o) return;
    o->k = 31;
    o->masks = 20000;            // index.go:560
    o->mask_seed = 1;
    o->max_desert = 100;         // index.go:582
    o->seed_dist = 50;           // index.go:584
    o->contig_interval = 1000;   // index.go:619
    o->genome_batch_size = 5000; // index.go:613
    o->max_genome = 20000000;    // index.go:538
}

// lm_index_builder_new (masks == nullptr: the generated set of bo->masks masks from bo->mask_seed) and
// lm_index_builder_new_masks (the caller's set: nmasks rules, bo->masks is ignored, bo->mask_seed is only carried to info.toml)
static lm_status builder_new(const char *who, const lm_build_opt *bo_in, const uint64_t *masks, size_t nmasks, const lm_options *opt,
                             const lm_residency *res, int device, lm_index_builder **out) {
    if (!out) return LM_ERR_ARG;
    *out = nullptr;
    if (!bo_in || !opt) {
        g_open_error = std::string(who) + ": build options and search options are needed";
        return LM_ERR_ARG;
    }
    lm_res_request rq;
    {
        const lm_status rs = lm_res_resolve(res, rq, g_open_error);
        if (rs != LM_OK) return rs;
    }
    lm_build_opt bo_copy = *bo_in;
    if (masks) {
        // (the set by the mask rule's own text, before the count is narrowed to the int of lm_build_opt and before any device is asked for)
        MaskPlan mp;
        std::string why;
        if (!plan_masks(bo_in->k, masks, nmasks, mp, why)) {
            g_open_error = std::string(who) + ": the mask set cannot be built with: " + why;
            return LM_ERR_ARG;
        }
        bo_copy.masks = (int32_t)nmasks;
    }
    const lm_build_opt *bo = &bo_copy;
    if (!build_opt_ok(who, *bo, masks == nullptr, g_open_error)) return LM_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        g_open_error = "no HIP device available (this library has no CPU path)";
        return LM_ERR_NO_DEVICE;
    }
    std::unique_ptr<lm_index_builder> b(new lm_index_builder());
    b->bo = *bo;
    b->rq = rq;
    // measurement / tests only; results do not depend on it
    if (const char *e = getenv("LM_BUILD_SLAB_KB")) b->slab_bytes = std::max<int64_t>(64, atoll(e)) << 10; // many small slabs
    try {
        lm_index *ix = new lm_index();
        b->ix = ix;
        ix->opt = *opt;
        ix->device = device;
        const lm_status hs = builder_header(who, ix, bo->k, bo->masks, bo->mask_seed, bo->contig_interval, nullptr, masks, b->pfx);
        if (hs != LM_OK) return hs;
    } catch (const std::exception &e) {
        g_open_error = e.what();
        return LM_ERR_HIP;
    }
    *out = b.release();
    return LM_OK;
}
lm_status lm_index_builder_new(const lm_build_opt *bo, const lm_options *opt, const lm_residency *res, int device, lm_index_builder **out) {
    return builder_new("lm_index_builder_new", bo, nullptr, 0, opt, res, device, out);
}
lm_status lm_index_builder_new_masks(const lm_build_opt *bo, const uint64_t *masks, size_t nmasks, const lm_options *opt, const lm_residency *res,
                                     int device, lm_index_builder **out) {
    if (!masks) {
        if (out) *out = nullptr;
        g_open_error = "lm_index_builder_new_masks: a mask set is needed";
        return LM_ERR_ARG;
    }
    return builder_new("lm_index_builder_new_masks", bo, masks, nmasks, opt, res, device, out);
}
// A builder that continues a resident index ("Adding genomes to a resident index").  Everything per record -
// key, captures, desert seeds, reversed seeds - is a function of the record and its number alone, and the packer takes seeds
// in any order: so the base's seeds are decoded from its image (k_sp_dump_range), the added records are captured, and finish()
// packs both into the image one build of all the genomes would have given.  Here: the settings, the check that the base's
// batches can be continued, and the base's host tables copied in front of what add() appends.
// lm_index_builder_like shares all of it but the base: the masks, options, device and build settings of `model`, no record.
static lm_status builder_from_model(const char *who, lm_index *base, bool continued, const lm_build_opt *bo_in, const lm_residency *res,
                                    lm_index_builder **out) {
    if (!out) return LM_ERR_ARG;
    *out = nullptr;
    const std::string w(who);
    if (!base) {
        g_open_error = w + (continued ? ": an index to continue is needed" : ": an index to take the settings from is needed");
        return LM_ERR_ARG;
    }
    lm_res_request rq;
    {
        const lm_status rs = lm_res_resolve(res, rq, g_open_error);
        if (rs != LM_OK) return rs;
    }
    std::lock_guard<std::mutex> base_lock(base->mu);
    const HostIndex &bh = base->host;
    lm_build_opt bo;
    lm_build_opt_default(&bo);
    if (bo_in) {
        const char *field = bo_in->k != bh.k                                   ? "k"
                            : bo_in->masks != bh.M                             ? "masks"
                            : bo_in->contig_interval != bh.contig_interval     ? "contig_interval"
                            : bo_in->genome_batch_size != bh.genome_batch_size ? "genome_batch_size"
                                                                               : nullptr;
        if (field) {
            g_open_error = w + ": " + field + " of the build options differs from the index that is " + (continued ? "continued" : "the model");
            return LM_ERR_ARG;
        }
        bo = *bo_in;
    } else {
        bo.max_desert = bh.max_seed_dist;
        bo.seed_dist = bh.seed_dist_in_desert;
    }
    bo.k = bh.k;
    bo.masks = bh.M;
    bo.mask_seed = bh.rand_seed; // (the masks are the base's, whatever seed made them)
    bo.contig_interval = bh.contig_interval;
    bo.genome_batch_size = bh.genome_batch_size;
    if (!build_opt_ok(who, bo, false, g_open_error)) return LM_ERR_ARG; // (the masks are the index's own: any k and shape the rule accepts)
    int64_t base_records = 0, nbase = 0;
    if (continued) {
        if (bh.synthetic && bh.shard_count > 1) {
            g_open_error = w + ": a shard of a synthetic set cannot be continued (its records are numbered without a table)";
            return LM_ERR_ARG;
        }
        // record n lies in batch n / genome_batch_size: every batch of the base but the last must be full
        const int nb = bh.genome_batches;
        bool regular = nb >= 1 && (int)bh.batch_first.size() == nb + 1 && bh.batch_first[0] == 0;
        for (int i = 0; regular && i < nb; i++) {
            const int64_t n = bh.batch_first[(size_t)i + 1] - bh.batch_first[(size_t)i];
            regular = i + 1 < nb ? n == bo.genome_batch_size : (n >= 1 && n <= bo.genome_batch_size);
        }
        if (!regular) {
            g_open_error = w + ": the genome batches of the index are irregular (not every batch but the last holds genome_batch_size = " +
                           std::to_string(bo.genome_batch_size) + " records, as in an index of the reference with split genomes): its records cannot be numbered on";
            return LM_ERR_ARG;
        }
        base_records = bh.batch_first[(size_t)nb];
        nbase = (int64_t)bh.genomes.size();
        if (bh.shard_count > 1 ? (int64_t)bh.g2local.size() != base_records : nbase != base_records) {
            g_open_error = w + ": the record tables of the index do not agree with its batches";
            return LM_ERR_ARG;
        }
    }
    std::unique_ptr<lm_index_builder> b(new lm_index_builder());
    b->bo = bo;
    b->rq = rq;
    if (continued) {
        b->base = base;
        b->base_records = base_records;
        b->nrecords = base_records;
        b->ninput = bh.input_genomes > 0 ? bh.input_genomes : base_records;
        b->input_bases = bh.total_bases;
    }
    if (const char *e = getenv("LM_BUILD_SLAB_KB")) b->slab_bytes = std::max<int64_t>(64, atoll(e)) << 10;
    try {
        lm_index *ix = new lm_index();
        b->ix = ix;
        ix->opt = base->opt;
        ix->device = base->device;
        const lm_status hs = builder_header(who, ix, bh.k, bh.M, bh.rand_seed, bh.contig_interval, &bh, nullptr, b->pfx);
        if (hs != LM_OK) return hs;
        HostIndex &h = ix->host;
        h.rand_seed = bh.rand_seed;
        h.max_seed_dist = bh.max_seed_dist;
        h.seed_dist_in_desert = bh.seed_dist_in_desert;
        if (continued) {
            // the base's tables in front: add() appends to them as it does in a fresh builder
            h.genomes = bh.genomes;
            h.others = bh.others;
            h.other_of = bh.other_of;
            h.chunk_of = bh.chunk_of;
            for (const auto &kv : bh.chunk_of) b->nlists = std::max(b->nlists, kv.second.list + 1);
            if (h.shard_count > 1) b->g2local = bh.g2local;
            b->reg_off.assign((size_t)nbase + 1, 0); // (no skip regions are needed for records that are not captured again)
            b->borrowed.assign((size_t)nbase, 1);
            lm_index_builder::Source S;
            S.ix = base; // (its records keep their keys: no rewrite table)
            for (int64_t l = 0; l < nbase; l++) {
                HostGenome &G = h.genomes[(size_t)l];
                G.bits_off = b->store_bytes; // its slot in the new store, filled by finish()
                b->store_bytes += build_slot_bytes(G.len);
                b->max_len = std::max<int64_t>(b->max_len, G.len);
                S.recs.emplace_back(l, l);
            }
            b->sources.push_back(std::move(S));
        }
    } catch (const std::exception &e) {
        g_open_error = e.what();
        return LM_ERR_HIP;
    }
    *out = b.release();
    return LM_OK;
}
lm_status lm_index_builder_extend(lm_index *base, const lm_build_opt *bo, const lm_residency *res, lm_index_builder **out) {
    return builder_from_model("lm_index_builder_extend", base, true, bo, res, out);
}
lm_status lm_index_builder_like(const lm_index *model, const lm_build_opt *bo, const lm_residency *res, lm_index_builder **out) {
    return builder_from_model("lm_index_builder_like", const_cast<lm_index *>(model), false, bo, res, out); // (its lock is taken; nothing of it is written)
}

// The records of a resident index appended to the builder ("Joining and subsetting resident indexes"): the
// checks, the plan (lm_join_plan.h) and copies of the source's host tables under the new keys.  No device work happens here;
// finish() copies the 2-bit records and decodes the seeds.
lm_status lm_index_builder_add_index(lm_index_builder *b, lm_index *src, const uint64_t *keep, size_t nkeep) {
    if (!b) return LM_ERR_ARG;
    if (b->broken) {
        b->err = "lm_index_builder_add_index: an earlier device error left this builder unusable: " + b->err;
        return LM_ERR_HIP;
    }
    auto refuse = [&](const std::string &why) {
        b->err = "lm_index_builder_add_index: " + why;
        return LM_ERR_ARG;
    };
    if (!src) return refuse("a source index is needed");
    lm_index *ix = b->ix;
    HostIndex &h = ix->host;
    if (src == b->base) return refuse("the source is the index this builder continues: its records are there already");
    for (const auto &S : b->sources)
        if (S.ix == src) return refuse("this source was added to the builder before");
    if (h.shard_count > 1) return refuse("the builder is sharded (shard_count = " + std::to_string(h.shard_count) + "): joining shards is not supported");
    std::lock_guard<std::mutex> src_lock(src->mu);
    const HostIndex &sh = src->host;
    if (sh.shard_count > 1) return refuse("the source is shard " + std::to_string(sh.shard_rank) + " of " + std::to_string(sh.shard_count) + ": joining shards is not supported");
    if (src->device != ix->device) return refuse("the source is on device " + std::to_string(src->device) + ", the builder on device " + std::to_string(ix->device));
    if (sh.k != h.k) return refuse("k differs: the source has " + std::to_string(sh.k) + ", the builder " + std::to_string(h.k));
    if (sh.contig_interval != h.contig_interval)
        return refuse("contig_interval differs: the source has " + std::to_string(sh.contig_interval) + ", the builder " + std::to_string(h.contig_interval));
    if (sh.M != h.M) return refuse("the number of masks differs: the source has " + std::to_string(sh.M) + ", the builder " + std::to_string(h.M));
    for (int i = 0; i < h.M; i++)
        if (sh.masks[(size_t)i] != h.masks[(size_t)i])
            return refuse("the mask values differ (first at mask " + std::to_string(i) + "): the two mask sets were not made from the same seed");
    if ((int64_t)sh.genomes.size() != src->view.ngenomes || src->view.shard_count > 1 || src->view.g2local)
        return refuse("the record tables of the source do not agree with its image");
    std::vector<JoinSrcRecord> table(sh.genomes.size());
    for (size_t l = 0; l < sh.genomes.size(); l++) {
        table[l].key = sh.genomes[l].bg;
        const auto it = sh.chunk_of.find(sh.genomes[l].bg);
        if (it != sh.chunk_of.end() && it->second.n > 1) {
            table[l].list = it->second.list;
            table[l].list_n = it->second.n;
            table[l].list_idx = it->second.idx;
        }
    }
    JoinPlan plan;
    std::string why;
    if (plan_join(table, keep, nkeep, b->nrecords, b->bo.genome_batch_size, b->nlists, plan, why) != JOIN_OK) return refuse(why);
    for (const JoinKept &k : plan.kept)
        if (sh.genomes[(size_t)k.src_local].len >= (1 << 28)) return refuse("a record of the source has 2^28 bases or more");
    // (the captured records so far lie in slabs that are consecutive pieces of the store: the slots of the borrowed records
    // come behind them, so the next captured record opens a new slab)
    if (!b->slabs.empty()) b->slabs.back()->cap = b->slabs.back()->used;
    lm_index_builder::Source S;
    S.ix = src;
    S.drops = plan.drops;
    for (const JoinKept &k : plan.kept) {
        HostGenome G = sh.genomes[(size_t)k.src_local]; // id, contig ids and sizes, genome_size, len, nseqs
        G.bg = k.key;
        G.global = k.number;
        G.bits_off = b->store_bytes; // its slot in the new store, filled by finish()
        b->store_bytes += build_slot_bytes(G.len);
        b->max_len = std::max<int64_t>(b->max_len, G.len);
        b->input_bases += G.genome_size;
        if (k.list >= 0) h.chunk_of[k.key] = HostIndex::ChunkInfo{k.list, k.list_n, k.list_idx};
        S.recs.emplace_back(k.src_local, (int64_t)h.genomes.size());
        b->reg_off.push_back((int32_t)b->reg_s.size()); // (no skip regions: the record is not captured)
        b->borrowed.push_back(1);
        h.genomes.push_back(std::move(G));
    }
    S.new_bg = std::move(plan.new_bg);
    b->sources.push_back(std::move(S));
    b->nrecords += (int64_t)plan.kept.size();
    b->ninput += plan.ninput;
    b->nlists = plan.nlists;
    return LM_OK;
}

lm_status lm_index_builder_add(lm_index_builder *b, const char *genome_id, const lm_contig *contigs, size_t ncontigs) {
    if (!b) return LM_ERR_ARG;
    if (b->broken) {
        b->err = "lm_index_builder_add: an earlier device error left this builder unusable: " + b->err;
        return LM_ERR_HIP;
    }
    if (!genome_id || (!contigs && ncontigs > 0)) {
        b->err = "lm_index_builder_add: genome id and contigs are needed";
        return LM_ERR_ARG;
    }
    for (size_t i = 0; i < ncontigs; i++)
        if (!contigs[i].id || (!contigs[i].seq && contigs[i].len > 0)) {
            b->err = std::string("lm_index_builder_add: contig without id or sequence in genome ") + genome_id;
            return LM_ERR_ARG;
        }
    lm_index *ix = b->ix;
    HostIndex &h = ix->host;
    const lm_build_opt &bo = b->bo;
    std::vector<uint32_t> lens(ncontigs);
    std::vector<const uint8_t *> seqs(ncontigs);
    int64_t bases = 0;
    for (size_t i = 0; i < ncontigs; i++) {
        lens[i] = contigs[i].len;
        seqs[i] = contigs[i].seq;
        bases += contigs[i].len;
    }
    std::vector<BuildRecord> recs;
    const int rc = plan_genome_records(lens.data(), ncontigs, bo.k, bo.contig_interval, bo.max_genome, recs);
    if (rc != BUILD_OK) {
        const int64_t maxg = bo.max_genome > 0 ? bo.max_genome : ((int64_t)1 << 28) - 1;
        b->err = std::string("genome ") + genome_id + " not added: " +
                 (rc == BUILD_NO_CONTIG    ? std::string("it has no contig")
                  : rc == BUILD_BIG_CONTIG ? "skipping a big genome with a sequence longer than max_genome (" + std::to_string(maxg) + " bp)"
                  : rc == BUILD_SHORT      ? "a genome record shorter than k = " + std::to_string(bo.k) + " bases"
                                           : std::string("a genome record of 2^28 bases or more"));
        return LM_ERR_ARG;
    }
    const bool keep = build_shard_keeps(b->nrecords, h.shard_count, h.shard_rank);
    // the device work of every record first, then the tables: a failure leaves nothing of the genome behind
    std::vector<int64_t> offs(recs.size(), 0);
    std::vector<std::vector<BuildRegion>> regs(recs.size());
    if (keep) {
        const size_t nslabs0 = b->slabs.size();
        const int64_t used0 = nslabs0 ? b->slabs.back()->used : 0, store0 = b->store_bytes;
        try {
            HIPCHK(hipSetDevice(ix->device));
            for (size_t r = 0; r < recs.size(); r++) {
                offs[r] = builder_pack(b, recs[r], contigs);
                plan_skip_regions(recs[r], seqs.data(), lens.data(), bo.contig_interval, regs[r]);
            }
        } catch (const std::exception &e) {
            b->err = e.what();
            if (hipStreamSynchronize(ix->lane[0].main.st) != hipSuccess) b->broken = true;
            (void)hipGetLastError();
            b->slabs.resize(nslabs0);
            if (nslabs0) b->slabs.back()->used = used0;
            b->store_bytes = store0;
            return dynamic_cast<const DeviceOOM *>(&e) ? LM_ERR_NOMEM : LM_ERR_HIP;
        }
    }
    for (size_t r = 0; r < recs.size(); r++) {
        const BuildRecord &R = recs[r];
        HostGenome G;
        G.bg = build_genome_key(b->nrecords, bo.genome_batch_size);
        G.global = b->nrecords;
        G.id = genome_id;
        G.genome_size = (int32_t)R.bases;
        G.len = R.len;
        G.nseqs = R.n;
        for (int c = 0; c < R.n; c++) {
            G.seq_sizes.push_back((int32_t)contigs[R.first + c].len);
            G.seq_ids.emplace_back(contigs[R.first + c].id);
        }
        if (recs.size() > 1) h.chunk_of[G.bg] = HostIndex::ChunkInfo{b->nlists, (int)recs.size(), (int)r};
        if (h.shard_count > 1) b->g2local.push_back(keep ? (int32_t)h.genomes.size() : -1);
        if (keep) {
            G.bits_off = offs[r];
            for (const BuildRegion &g : regs[r]) {
                b->reg_s.push_back(g.s);
                b->reg_e.push_back(g.e);
            }
            b->reg_off.push_back((int32_t)b->reg_s.size());
            b->max_len = std::max<int64_t>(b->max_len, R.len);
            b->borrowed.push_back(0);
            h.genomes.push_back(std::move(G));
        } else {
            G.bits_off = -1;
            h.other_of[G.bg] = (int)h.others.size();
            h.others.push_back(std::move(G));
        }
        b->nrecords++;
    }
    if (recs.size() > 1) b->nlists++;
    b->ninput++;
    b->input_bases += bases;
    return LM_OK;
}

lm_status lm_index_builder_finish(lm_index_builder *bp, lm_index **out) {
    if (out) *out = nullptr;
    std::unique_ptr<lm_index_builder> b(bp); // consumed whatever happens
    if (!bp || !out) return LM_ERR_ARG;
    if (b->broken) {
        g_open_error = "lm_index_builder_finish: an earlier device error left this builder unusable: " + b->err;
        return LM_ERR_HIP;
    }
    if (b->nrecords == b->base_records || b->ix->host.genomes.empty()) {
        g_open_error = b->nrecords == b->base_records ? "lm_index_builder_finish: no genome was added" : "lm_index_builder_finish: no genome of this shard was added";
        return LM_ERR_ARG;
    }
    // (the builder reads the images and stores of the base and of every source: no search or save of them runs meanwhile.  The
    // locks are taken in the order of the handles' addresses, so that two finishes that share sources cannot wait for each other)
    std::vector<lm_index *> held;
    for (const auto &S : b->sources) held.push_back(S.ix);
    std::sort(held.begin(), held.end(), std::less<lm_index *>());
    held.erase(std::unique(held.begin(), held.end()), held.end());
    std::vector<std::unique_lock<std::mutex>> src_locks;
    for (lm_index *p : held) src_locks.emplace_back(p->mu);
    try {
        HIPCHK(hipSetDevice(b->ix->device));
        builder_finish(b.get());
    } catch (const DeviceOOM &e) {
        g_open_error = e.what();
        if (b->sources.size() > (b->base ? 1u : 0u))
            g_open_error = "lm_index_builder_finish: the images and stores of the " + std::to_string(b->sources.size()) + " resident indexes that are read" +
                           ", the new store, the new image and the seed staging do not fit the device together (the sources are intact): " + g_open_error;
        else if (b->base)
            g_open_error = "lm_index_builder_finish: the base's image, the extended image and the seed staging do not fit the device together (the base is "
                           "intact): " + g_open_error;
        return LM_ERR_NOMEM;
    } catch (const std::exception &e) {
        g_open_error = e.what();
        return LM_ERR_HIP;
    }
    *out = b->ix;
    b->ix = nullptr;
    return LM_OK;
}

void lm_index_builder_free(lm_index_builder *b) { delete b; }

const char *lm_index_builder_last_error(const lm_index_builder *b) { return b ? b->err.c_str() : g_open_error.c_str(); }

lm_status lm_index_build_synthetic(const lm_synth_spec *spec, const lm_options *opt, int device, lm_index **out) {
    return lm_index_build_synthetic_ex(spec, opt, nullptr, device, out);
}
// The synthetic front end: the genomes of this shard written straight into one store (no slabs: the peak of a build is the
// store + the staging of one chunk), their names and keys; the records of a sharded set are numbered without a table
// (h.g2local stays empty).  Chunks of 2048 records whatever their length: at 5 Mb per genome that is eight full rounds of one
// workgroup per CU, where a bound on the bases would leave CUs idle and multiply the host synchronisations.
lm_status lm_index_build_synthetic_ex(const lm_synth_spec *spec, const lm_options *opt, const lm_residency *res, int device, lm_index **out) {
    *out = nullptr;
    lm_res_request rq;
    {
        const lm_status rs = lm_res_resolve(res, rq, g_open_error);
        if (rs != LM_OK) return rs;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_open_error = "no HIP device available (this library has no CPU path)";
        return LM_ERR_NO_DEVICE;
    }
    if (!seed_settings_ok("lm_index_build_synthetic", spec->k, spec->masks, spec->max_desert, spec->seed_dist, true, g_open_error)) return LM_ERR_ARG;
    if (spec->genome_len < 64 || spec->genomes < 1 || spec->genome_len >= (1 << 28) || spec->families < 1) {
        g_open_error = "lm_index_build_synthetic: unsupported spec (genome_len in [64, 2^28), genomes and families >= 1)";
        return LM_ERR_ARG;
    }
    lm_index *ix = new lm_index();
    try {
        ix->opt = *opt;
        ix->device = device;
        std::vector<int32_t> pfx;
        const lm_status hs = builder_header("lm_index_build_synthetic", ix, spec->k, spec->masks, spec->mask_seed, 1000, nullptr, nullptr, pfx);
        if (hs != LM_OK) {
            delete ix;
            return hs;
        }
        HostIndex &h = ix->host;
        h.synthetic = true;
        h.synth_genome_len = spec->genome_len;
        h.synth_genomes = spec->genomes;
        h.total_bases = opt->total_bases_override > 0 ? opt->total_bases_override : spec->genomes * (int64_t)spec->genome_len;
        h.genome_batches = (int)((spec->genomes + 4999) / 5000);
        h.batch_first.assign(h.genome_batches + 1, 0);
        for (int b = 0; b <= h.genome_batches; b++) h.batch_first[b] = std::min<int64_t>((int64_t)b * 5000, spec->genomes);
        // local genomes
        int64_t nlocal = 0;
        for (int64_t g = 0; g < spec->genomes; g++)
            if ((int)(g % h.shard_count) == h.shard_rank) nlocal++;
        SynthDev sp;
        sp.seed = (uint64_t)spec->seed;
        sp.genomes = spec->genomes;
        sp.genome_len = spec->genome_len;
        sp.families = (int32_t)std::min<int64_t>(spec->families, spec->genomes);
        sp.max_div = spec->max_div;
        sp.shard_rank = h.shard_rank;
        sp.shard_count = h.shard_count;
        sp.nlocal = nlocal;
        sp.nblk = (spec->genome_len + 511) >> 9;
        sp.gbytes = build_slot_bytes(spec->genome_len);
        ix->d_gbits.alloc_exact((size_t)(nlocal * sp.gbytes) + 64);
        HIPCHK(hipMemsetAsync(ix->d_gbits.p, 0, (size_t)(nlocal * sp.gbytes) + 64, ix->lane[0].main.st));
        DBuf<int16_t> shifts;
        shifts.ensure((size_t)(nlocal * sp.nblk) + 1);
        hipLaunchKernelGGL(k_synth_shifts, dim3(gridn(nlocal, 64)), dim3(64), 0, ix->lane[0].main.st, sp, shifts.p);
        hipLaunchKernelGGL(k_synth_genomes, dim3(gridn(nlocal * (((int64_t)spec->genome_len + 3) >> 2))), dim3(256), 0, ix->lane[0].main.st,
                           sp, shifts.p, ix->d_gbits.p);
        bsync(ix);
        shifts.release();
        h.genomes.resize(nlocal);
        for (int64_t l = 0; l < nlocal; l++) {
            int64_t g = h.shard_count > 1 ? l * h.shard_count + h.shard_rank : l;
            HostGenome &G = h.genomes[l];
            G.bg = build_genome_key(g, 5000);
            G.global = g;
            char nm[64];
            snprintf(nm, sizeof nm, "SYN_%09lld.1", (long long)g);
            G.id = nm;
            G.genome_size = spec->genome_len;
            G.len = spec->genome_len;
            G.nseqs = 1;
            G.seq_sizes = {spec->genome_len};
            snprintf(nm, sizeof nm, "syn%09lld_c1", (long long)g);
            G.seq_ids = {std::string(nm)};
            G.bits_off = l * sp.gbytes;
        }
        const std::vector<int32_t> no_regions((size_t)nlocal + 1, 0);
        build_seed_index(ix, pfx, no_regions, {}, {}, spec->max_desert, spec->seed_dist, 2048, INT64_MAX, {}, {}, rq);
    } catch (const PinnedOOM &e) {
        g_open_error = e.what();
        delete ix;
        return LM_ERR_NOMEM;
    } catch (const std::exception &e) {
        g_open_error = e.what();
        delete ix;
        return LM_ERR_HIP;
    }
    *out = ix;
    return LM_OK;
}
lm_status lm_index_fetch(lm_index *ix, int64_t local_genome, int64_t start, int64_t len, uint8_t *out) {
    if (!ix || local_genome < 0 || local_genome >= (int64_t)ix->host.genomes.size()) return LM_ERR_ARG;
    const HostGenome &G = ix->host.genomes[local_genome];
    if (start < 0 || len < 0 || start + len > G.len) return LM_ERR_ARG;
    try {
        std::lock_guard<std::mutex> lock(ix->mu);
        HIPCHK(hipSetDevice(ix->device));
        DBuf<uint8_t> d;
        d.ensure((size_t)len + 1);
        // (a host-resident genome is read where it lives: lm_kernels.hip, k_stage_genome_bits, lists the kernels that may)
        const uint8_t *gsrc = !ix->g_hptr.empty() && ix->g_hptr[(size_t)local_genome] ? ix->g_hptr[(size_t)local_genome] : ix->d_gbits.p + G.bits_off;
        hipLaunchKernelGGL(k_fetch_bases, dim3(gridn(len)), dim3(256), 0, ix->lane[0].main.st, gsrc, start, len, d.p);
        HIPCHK(hipMemcpyAsync(out, d.p, (size_t)len, hipMemcpyDeviceToHost, ix->lane[0].main.st));
        bsync(ix);
    } catch (const std::exception &e) {
        ix->err = e.what();
        return LM_ERR_HIP;
    }
    return LM_OK;
}

} // extern "C"

// The window records of genome screening packed in ONE launch (k_pack_record packs one record of several contigs; here every
// record is one stretch of `ascii` and there may be queries x windows of them): one lane per byte of the store, which finds its
// record by the slot offsets goff (ascending, the slots back to back) and packs four bases with the builder's base table,
// first base in bits 7-6.  Bytes behind a record's last base (the slot's padding) are left as they are: zero.
namespace lm {
__global__ void k_pack_windows(const uint8_t *__restrict__ ascii, const int64_t *__restrict__ src_off, const int64_t *__restrict__ goff,
                               const int32_t *__restrict__ len, int64_t nrec, int64_t store, uint8_t *__restrict__ out) {
    for (int64_t by = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; by < store; by += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = 0, hi = nrec; // the last record whose slot starts at or before this byte
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if (goff[mid] <= by) lo = mid;
            else hi = mid;
        }
        const int64_t i0 = (by - goff[lo]) << 2;
        const int64_t n = len[lo];
        if (i0 >= n) continue;
        uint32_t v = 0;
        for (int j = 0; j < 4; j++) v = (v << 2) | (i0 + j < n ? build_base_code(ascii[src_off[lo] + i0 + j]) : 0u);
        out[by] = (uint8_t)v;
    }
}
} // namespace lm

// Genome screening's capture (lm_screen.hip), through the builder's store code and k_capture_g: "record" r is the window
// ascii[src_off[r] .. + len[r]) of a query genome's concatenation (device memory), packed on its own by k_pack_windows so that
// it starts on a slot boundary, and captured by one workgroup with the skip regions reg_s / reg_e [reg_off[r], reg_off[r + 1])
// - in the window's own coordinates, whatever the caller means by them.  d_kmers[r * M + m] receives the k-mer mask m
// captures in record r with the missing-prefix rule (check_shorter), 0 where there is none or it is of low complexity.  At
// most 1024 records per launch: with the minima in a global table a record of a launch costs 8 B x masks of scratch.
void lm::lm_screen_capture(lm_index *ix, hipStream_t st, const uint8_t *d_ascii, const std::vector<int64_t> &src_off,
                           const std::vector<int32_t> &len, const std::vector<int32_t> &reg_off, const std::vector<int32_t> &reg_s,
                           const std::vector<int32_t> &reg_e, uint64_t *d_kmers) {
    const HostIndex &h = ix->host;
    const int K = h.k, M = h.M, p = h.mask_prefix;
    const int64_t nrec = (int64_t)len.size();
    if (nrec == 0) return;
    std::vector<int32_t> pfx(((size_t)1 << (2 * p)) + 1, 0);
    for (int m = 0; m < M; m++) pfx[(size_t)(h.masks[(size_t)m] >> ((K - p) << 1)) + 1]++;
    for (size_t f = 1; f < pfx.size(); f++) pfx[f] += pfx[f - 1];
    const CapturePlan cp = capture_plan(M, p, pfx);
    const auto capture = capture_kernel<true>(cp);
    if (cp.lds_bytes > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)capture, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cp.lds_bytes));
    std::vector<int64_t> goff((size_t)nrec);
    int64_t store = 0;
    for (int64_t r = 0; r < nrec; r++) {
        goff[(size_t)r] = store;
        store += build_slot_bytes(len[(size_t)r]);
    }
    auto up = [&](auto &dbuf, const auto &vec) {
        dbuf.alloc_exact(std::max<size_t>(vec.size(), 1));
        if (!vec.empty()) HIPCHK(hipMemcpyAsync(dbuf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, st));
    };
    DBuf<uint8_t> bits;
    DBuf<int64_t> d_goff, d_src;
    DBuf<int32_t> d_len, d_reg_off, d_reg_s, d_reg_e;
    DBuf<uint64_t> dbl_map;
    DBuf<uint32_t> dbl_cnt;
    DBuf<unsigned long long> hashes;
    bits.alloc_exact((size_t)store, true, st);
    up(d_goff, goff);
    up(d_src, src_off);
    up(d_len, len);
    up(d_reg_off, reg_off);
    up(d_reg_s, reg_s);
    up(d_reg_e, reg_e);
    up(dbl_map, cp.dmap);
    up(dbl_cnt, cp.dcnt);
    const int64_t per_launch = 1024;
    hashes.alloc_exact(cp.lds_capture ? 1 : (size_t)std::min(nrec, per_launch) * M);
    hipLaunchKernelGGL(k_pack_windows, dim3(gridn(store)), dim3(256), 0, st, d_ascii, d_src.p, d_goff.p, d_len.p, nrec, store, bits.p);
    HIPCHK(hipGetLastError());
    const MaskTab mt{ix->d_masks.p, ix->d_pfx_first.p, K, p, M};
    const GenomeTab gt{d_goff.p, d_len.p, nullptr, d_reg_off.p, d_reg_s.p, d_reg_e.p};
    for (int64_t r0 = 0; r0 < nrec; r0 += per_launch) {
        const int n = (int)std::min(per_launch, nrec - r0);
        hipLaunchKernelGGL(capture, dim3(n), dim3(1024), cp.lds_bytes, st, gt, mt, bits.p, r0, dbl_map.p, dbl_cnt.p, hashes.p, (uint32_t *)nullptr,
                           (uint32_t *)nullptr, (uint16_t *)nullptr, d_kmers + r0 * M, (uint64_t *)nullptr, (unsigned long long *)nullptr, 0ull,
                           (uint64_t *)nullptr, (unsigned long long *)nullptr, 0ull, (unsigned long long *)nullptr);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(st)); // (the tables and the store above go out of scope)
}
