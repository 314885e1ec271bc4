// lm_screen.hip — genome screening on the device: lm_index_screen_genomes (include/lexicmap_hip.h).
// The first stage of `lexicmap genome search`, GSearchScreen (lib-index-search-genome.go:114-543), for a batch of query genomes.
//
//   pack + capture   the query genomes' windows are "records" of the builder: k_pack_record and k_capture_g<.., KM = true>
//                    (lm_builder.hip, lm_screen_capture) leave the k-mer every mask captures in every window - the missing-prefix
//                    rule applied, low-complexity captures zeroed.  As the reference does (:180), every window is masked with
//                    the UNSHIFTED skip regions of the whole sequence: the spacers' coordinates are taken as the window's own.
//   k_screen_prep    one lane per (window, mask): drops a k-mer an earlier window of the same query captured under the same
//                    mask (:197-204), classifies the rest as the read search does (partition of the packed forward list, or the
//                    flat outlier list, or nothing stored that could match) and appends (sort key, slot).  Forward lists only
//                    (Search2(.., checkFlag = true, reversedKmer = false), :371).  The key starts with the MASK, so after the
//                    radix sort the lookups of a mask are together.
//   k_screen_count   one lane per sorted lookup: the range [kmer & ~low, kmer | low] in its partition or outlier list
//                    (kv-searcher2.go:326-549), the values in it and how many of them the genome whitelist keeps, summed per mask.
//   pieces           the host cuts the masks into runs whose tuples fit the device (lm_screen_plan.h); per piece:
//   k_screen_emit    the lanes over the OUTPUT as in k_lookup_emit_flat: one stored value read, one tuple
//                    query | local record | mask | Len written (Len = LCP of the two k-mers, k when they are equal); a value
//                    the whitelist drops becomes an all-ones key that sorts behind the rest.
//   radix sort       of the tuples, then k_screen_flags + two scans number the (query, record, mask) and (query, record) groups,
//   k_screen_reduce  a lane walks 16 sorted tuples: Score += Len, Hits (saturating at 255: the 256th value of a group no longer
//                    counts) and Longest (the last tuple of a group) per mask, added to the row of the (query, record) with one
//                    set of atomics per row change - :316-341.
// The host adds the rows of the pieces up (a piece holds whole masks, so only sums meet), merges the records of split genomes,
// orders and cuts (lm_screen_plan.h).  Memory: 34 B per tuple of a piece (two 8-byte key arrays, two flag bytes, two 8-byte
// scans) plus the radix sort's scratch, 40 B per (query, record) row, 1 B per hit mask of a row.
// Shards: where a search starts is decided by a mask's whole list (screen_shadowed), of which a shard holds its own records'
// part; lm_index_screen_structure / lm_index_screen_add_structure carry the rest between the ranks (ScreenShadowTab).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "lm_internal.h"
#include "lm_lookup_dev.h"
#include "lm_merge.h"
#include "lm_prims.h"
#include "lm_screen_plan.h"

namespace lm {

#define SC_LEN_BITS 6   /* Len <= 32 */
#define SC_MASK_BITS 16 /* masks <= 65535 */
#define SC_REC_SHIFT (SC_LEN_BITS + SC_MASK_BITS)
#define SC_RUN 16       /* sorted tuples per lane of k_screen_reduce */

struct ScreenRowDev { // one (query, record) of a piece
    uint64_t key;     // query | local record
    unsigned long long score;
    uint32_t hit_masks, hit_kmers, score2, pad;
    uint64_t pref_first;
};

// sort key of a lookup: mask | outlier | partition.  pb = 2 * part_bases bits of partition.
__global__ __launch_bounds__(256) void k_screen_prep(DevIndexView ix, const uint64_t *__restrict__ kmers, const int32_t *__restrict__ rec_first,
                                                     int64_t nslots, uint32_t *__restrict__ keys, uint32_t *__restrict__ slots,
                                                     unsigned long long *__restrict__ counter) {
    const int pb = ix.part_bases << 1, p = ix.mask_prefix;
    const int lane = threadIdx.x & 63;
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < nslots; t0 += (int64_t)gridDim.x * blockDim.x) { // (wave-uniform trip count)
        const int64_t t = t0 + threadIdx.x;
        uint32_t key = 0xffffffffu;
        if (t < nslots) {
            const uint64_t x = kmers[t];
            const int64_t r = t / ix.M;
            const int m = (int)(t - r * ix.M);
            bool use = x != 0;
            for (int64_t r2 = rec_first[r]; use && r2 < r; r2++) use = kmers[r2 * ix.M + m] != x; // an earlier window has it
            if (use) {
                if ((x >> ((ix.K - p) << 1)) == (ix.masks[m] >> ((ix.K - p) << 1))) {
                    key = ((uint32_t)m << (pb + 1)) | ((uint32_t)(x >> ix.key_bits) & (uint32_t)(ix.P1 - 2));
                } else if (ix.out_off[2 * m + 1] > ix.out_off[2 * m]) {
                    key = ((uint32_t)m << (pb + 1)) | (1u << pb);
                } // (else: nothing stored under this mask shares min_prefix >= p bases with x)
            }
        }
        const bool issue = key != 0xffffffffu;
        const unsigned long long b = __ballot(issue);
        unsigned long long base = 0;
        if (lane == 0 && b) base = atomicAdd(counter, (unsigned long long)__popcll(b));
        base = __shfl(base, 0, 64);
        if (issue) {
            const unsigned long long o = base + (unsigned long long)__popcll(b & ((1ull << lane) - 1));
            keys[o] = key;
            slots[o] = (uint32_t)t;
        }
    }
}

// (screen_shadowed, ScreenShadowTab - the reference's anchor-index start rule - live in lm_lookup_dev.h: the read search applies
// the same rule)

// the occupied partitions of every list: bits[md * W + w] bit b = partition w * 64 + b of list md holds a seed
__global__ void k_screen_occupancy(DevIndexView ix, int W, uint64_t *__restrict__ bits) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)2 * ix.M * W) return;
    const int64_t md = t / W;
    const int w = (int)(t - md * W);
    const uint32_t *row = ix.part_tab + md * ix.P1;
    uint64_t v = 0;
    for (int b = 0; b < 64; b++) {
        const int A = w * 64 + b;
        if (A < ix.P1 - 1 && row[A + 1] > row[A]) v |= 1ull << b;
    }
    bits[t] = v;
}

// per_mask: [3][M] values in range, values the whitelist keeps, lookups
__global__ __launch_bounds__(256) void k_screen_count(DevIndexView ix, const uint64_t *__restrict__ kmers, const uint32_t *__restrict__ skeys,
                                                      const uint32_t *__restrict__ sslots, int64_t nlk, int min_prefix,
                                                      uint32_t *__restrict__ counts, int64_t *__restrict__ starts,
                                                      unsigned long long *__restrict__ per_mask, ScreenShadowTab tab) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = j < nlk;
    const int pb = ix.part_bases << 1;
    const uint32_t sk = active ? skeys[j] : 0u;
    const uint32_t m = active ? sk >> (pb + 1) : 0xffffffffu; // (no mask: a segment of its own below)
    const uint64_t x = active ? kmers[sslots[j]] : 0ull;
    uint64_t left = 0, right = 0;
    lookup_range(x, ix.K, min_prefix, &left, &right);
    int64_t st = 0;
    int32_t nv = 0, kept = 0;
    if (!active) {
    } else if (!((sk >> pb) & 1u)) {
        const uint32_t part = sk & ((1u << pb) - 1);
        const uint32_t *row = ix.part_tab + (int64_t)(2 * m) * ix.P1 + part;
        const int64_t base = ix.md_off[2 * m];
        const uint64_t km = (1ull << ix.key_bits) - 1;
        nv = lm_partition_range(ix.pk_keys, ix.key_bits, base + row[0], base + row[1], left & km, right & km, &st);
        kept = nv;
        if (ix.g_keep && nv) {
            kept = 0;
            for (int32_t s = 0; s < nv; s++)
                kept += genome_kept(ix, (int64_t)lm_packed_val_genome(lm_bits_get(ix.pk_vals, st + s, ix.gid_bits + ix.pos_bits + 1), ix.pos_bits));
        }
    } else {
        int64_t lo = ix.out_off[2 * m], hi = ix.out_off[2 * m + 1];
        const int64_t e = hi;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (ix.out_kmers[mid] < left) lo = mid + 1;
            else hi = mid;
        }
        st = lo;
        while (lo < e && ix.out_kmers[lo] <= right) lo++;
        nv = (int32_t)(lo - st);
        for (int32_t s = 0; s < nv; s++) {
            const int g = local_genome(ix, ix.out_vals[st + s] >> 30);
            kept += g >= 0 && (!ix.g_keep || genome_kept(ix, g));
        }
    }
    if (nv && screen_shadowed(ix, tab, m, x, right)) nv = kept = 0; // (the reference's search starts behind the range)
    if (active) {
        counts[j] = (uint32_t)nv;
        starts[j] = st;
    }
    // The lookups are sorted by mask, so the lanes of a wavefront are a few runs of one mask each: the sums of a run are added
    // up across its lanes (a neighbour d lanes on with the same mask has only lanes of that mask in between) and the first
    // lane of the run issues the three atomics - one set per mask and wavefront instead of one per lookup.
    const int lane = threadIdx.x & 63;
    unsigned long long s_nv = (unsigned long long)nv, s_kept = (unsigned long long)kept, s_n = active ? 1ull : 0ull;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t m2 = __shfl_down(m, d, 64);
        const unsigned long long a = __shfl_down(s_nv, d, 64), b = __shfl_down(s_kept, d, 64), c = __shfl_down(s_n, d, 64);
        if (lane + d < 64 && m2 == m) {
            s_nv += a;
            s_kept += b;
            s_n += c;
        }
    }
    const uint32_t mprev = __shfl_up(m, 1, 64);
    if (active && (lane == 0 || mprev != m)) {
        if (s_nv) atomicAdd(&per_mask[m], s_nv);
        if (s_kept) atomicAdd(&per_mask[ix.M + m], s_kept);
        atomicAdd(&per_mask[2 * ix.M + m], s_n);
    }
}

// the tuples of the lookups [j0, j1): lookup j writes counts[j] of them at offs[j] - offs[j0]
__global__ __launch_bounds__(256) void k_screen_emit(DevIndexView ix, const uint64_t *__restrict__ kmers, const int32_t *__restrict__ rec2q,
                                                     const uint32_t *__restrict__ skeys, const uint32_t *__restrict__ sslots, int64_t j0,
                                                     int64_t j1, const uint32_t *__restrict__ counts, const int64_t *__restrict__ offs,
                                                     const int64_t *__restrict__ starts, int qshift, uint64_t *__restrict__ out) {
    const int64_t j = j0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int pb = ix.part_bases << 1;
    const int64_t piece_base = offs[j0];
    uint32_t cnt = 0, sk = 0, slot = 0;
    int64_t off = offs[j1] - piece_base, st = 0; // (lanes behind the last lookup: the end of the output, no tuples)
    uint64_t x = 0;
    if (j < j1) {
        cnt = counts[j];
        off = offs[j] - piece_base;
        if (cnt) {
            sk = skeys[j];
            slot = sslots[j];
            st = starts[j];
            x = kmers[slot];
        }
    }
    const int64_t wave_base = __shfl(off, 0, 64);
    const int64_t total = __shfl(off + (int64_t)cnt, 63, 64) - wave_base;
    const uint64_t km = (1ull << ix.key_bits) - 1;
    const int fixed = ix.K - (ix.key_bits >> 1); // p + a bases shared by construction
    const int64_t rel = off - wave_base;
    for (int64_t base = 0; base < total; base += 64) { // wave-uniform trip count: every lane takes part in the shuffles
        const int64_t o = base + (int64_t)(threadIdx.x & 63);
        int L = 0; // the last lane whose first tuple is <= o (lanes without tuples share their successor's offset)
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {
            const int64_t rc = __shfl(rel, L + step, 64); // (L + step <= 63)
            if (rc <= o) L += step;
        }
        const int64_t s = o - __shfl(rel, L, 64);
        const uint32_t sk_ = __shfl(sk, L, 64), slot_ = __shfl(slot, L, 64);
        const int64_t st_ = __shfl(st, L, 64);
        const uint64_t x_ = __shfl(x, L, 64);
        if (o < total) {
            const uint32_t r = slot_ / (uint32_t)ix.M;
            const uint32_t m = slot_ - r * (uint32_t)ix.M;
            int64_t g;
            int len;
            if (!((sk_ >> pb) & 1u)) {
                const uint64_t sr = lm_bits_get(ix.pk_keys, st_ + s, ix.key_bits);
                const uint64_t d = sr ^ (x_ & km);
                len = fixed + (d ? ((lm_clz64(d) - (64 - ix.key_bits)) >> 1) : (ix.key_bits >> 1));
                g = (int64_t)lm_packed_val_genome(lm_bits_get(ix.pk_vals, st_ + s, ix.gid_bits + ix.pos_bits + 1), ix.pos_bits);
            } else {
                g = local_genome(ix, ix.out_vals[st_ + s] >> 30);
                len = lm_lcp(x_, ix.out_kmers[st_ + s], ix.K);
            }
            const bool keep = g >= 0 && (!ix.g_keep || genome_kept(ix, g));
            out[wave_base + o] = keep ? ((uint64_t)rec2q[r] << qshift) | ((uint64_t)g << SC_REC_SHIFT) | ((uint64_t)m << SC_LEN_BITS) | (uint64_t)len
                                      : ~0ull;
        }
    }
}

// fm[i]: tuple i opens a (query, record, mask) group; fr[i]: a (query, record) group.  n + 1 entries, the last 0 (the scans' total)
__global__ void k_screen_flags(const uint64_t *__restrict__ keys, int64_t n, uint8_t *__restrict__ fm, uint8_t *__restrict__ fr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        fm[i] = fr[i] = 0;
        return;
    }
    const uint64_t k = keys[i], kp = i ? keys[i - 1] : ~k;
    fm[i] = (k >> SC_LEN_BITS) != (kp >> SC_LEN_BITS);
    fr[i] = (k >> SC_REC_SHIFT) != (kp >> SC_REC_SHIFT);
}

// om / orr: exclusive scans of fm / fr.  rows (zeroed) [orr[n]], prefs [om[n]] or null (details off)
__global__ __launch_bounds__(256) void k_screen_reduce(const uint64_t *__restrict__ keys, int64_t n, const uint8_t *__restrict__ fm,
                                                       const uint8_t *__restrict__ fr, const int64_t *__restrict__ om,
                                                       const int64_t *__restrict__ orr, ScreenRowDev *__restrict__ rows,
                                                       uint8_t *__restrict__ prefs) {
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * SC_RUN;
    if (i0 >= n) return;
    const int64_t i1 = i0 + SC_RUN < n ? i0 + SC_RUN : n;
    int rank = 0; // of tuple i0 in its (query, record, mask) group, 255 = that or more (fm[0] is set: the walk ends)
    for (int64_t j = i0; !fm[j] && rank < 255; j--) rank++;
    int64_t row = orr[i0] + fr[i0] - 1;
    unsigned long long sc = 0;
    uint32_t hm = 0, hk = 0, s2 = 0;
    auto flush = [&]() {
        if (sc) atomicAdd(&rows[row].score, sc);
        if (hm) atomicAdd(&rows[row].hit_masks, hm);
        if (hk) atomicAdd(&rows[row].hit_kmers, hk);
        if (s2) atomicAdd(&rows[row].score2, s2);
        sc = 0;
        hm = hk = s2 = 0;
    };
    for (int64_t i = i0; i < i1; i++) {
        const uint64_t k = keys[i];
        const uint32_t len = (uint32_t)(k & ((1u << SC_LEN_BITS) - 1));
        if (fr[i]) {
            if (i > i0) {
                flush();
                row++;
            }
            rows[row].key = k >> SC_REC_SHIFT;
            rows[row].pref_first = (uint64_t)om[i];
        }
        if (i > i0) rank = fm[i] ? 0 : (rank < 255 ? rank + 1 : 255);
        if (fm[i]) hm++;
        if (rank < 255) hk++; // Hits saturates at 255 (:329)
        sc += len;
        if (i + 1 == n || fm[i + 1]) { // the largest Len of the group: the tuples are sorted
            s2 += len;
            if (prefs) prefs[om[i] + fm[i] - 1] = (uint8_t)len;
        }
    }
    flush();
}

struct ScreenOut {
    std::vector<ScreenPartial> partials;
    std::vector<uint8_t> prefs;
    lm_screen_stats stats;
};

// queries [q0, q1) of the batch: partial sums per (query, record) and piece are appended to `out`
static void screen_sub_batch(lm_index *ix, const lm_genome_query *queries, const std::vector<ScreenLayout> &lay, size_t q0, size_t q1,
                             const lm_screen_opt &opt, ScreenOut &out) {
    const hipStream_t st = ix->lane[0].main.st;
    DBuf<uint8_t> &tmp = ix->lane[0].main.tmp;
    const HostIndex &h = ix->host;
    const DevIndexView &v = ix->view;
    const int K = h.k, M = h.M;
    const bool dbg = getenv("LM_DEBUG") != nullptr;
    const double t0 = now_ms();
    // ---- the concatenations (spacers of A: skipped anyway) and the window records
    std::vector<int64_t> qbase(q1 - q0 + 1, 0);
    for (size_t q = q0; q < q1; q++) qbase[q - q0 + 1] = qbase[q - q0] + lay[q].len;
    std::vector<uint8_t> ascii((size_t)qbase.back() + 1, (uint8_t)'A');
    std::vector<int64_t> src_off;
    std::vector<int32_t> len, reg_off(1, 0), reg_s, reg_e, rec2q, rec_first;
    std::vector<ScreenWindow> win;
    for (size_t q = q0; q < q1; q++) {
        const ScreenLayout &L = lay[q];
        for (size_t c = 0; c < queries[q].ncontigs; c++)
            if (queries[q].contigs[c].len) memcpy(ascii.data() + qbase[q - q0] + L.start[c], queries[q].contigs[c].seq, queries[q].contigs[c].len);
        screen_windows(L.len, opt.windows, win);
        const int32_t first = (int32_t)len.size();
        for (const ScreenWindow &w : win) {
            out.stats.windows++;
            if (w.len < K) continue; // no k-mer
            src_off.push_back(qbase[q - q0] + w.start);
            len.push_back((int32_t)w.len);
            rec2q.push_back((int32_t)q);
            rec_first.push_back(first);
            reg_s.insert(reg_s.end(), L.reg_s.begin(), L.reg_s.end()); // (:180: the whole sequence's regions, unshifted)
            reg_e.insert(reg_e.end(), L.reg_e.begin(), L.reg_e.end());
            reg_off.push_back((int32_t)reg_s.size());
        }
        out.stats.query_bases += L.len;
    }
    const int64_t nrec = (int64_t)len.size();
    if (nrec == 0) return;
    const int64_t nslots = nrec * M;
    auto up = [&](auto &dbuf, const auto &vec) {
        dbuf.alloc_exact(std::max<size_t>(vec.size(), 1));
        if (!vec.empty()) HIPCHK(hipMemcpyAsync(dbuf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, st));
    };
    DBuf<uint64_t> d_kmers;
    d_kmers.alloc_exact((size_t)nslots);
    {
        DBuf<uint8_t> d_ascii;
        up(d_ascii, ascii);
        lm_screen_capture(ix, st, d_ascii.p, src_off, len, reg_off, reg_s, reg_e, d_kmers.p);
    }
    const double t1 = now_ms();
    // ---- lookups: classify, sort by (mask, outlier, partition), count
    const int pb = v.part_bases << 1;
    if (SC_MASK_BITS + 1 + pb > 32) throw HipError("lm_index_screen_genomes: the partition index of this image is too wide for a 32-bit lookup key");
    DBuf<int32_t> d_rec2q, d_rec_first;
    up(d_rec2q, rec2q);
    up(d_rec_first, rec_first);
    DBuf<uint32_t> lk_key, lk_slot, lk_key2, lk_slot2, counts;
    DBuf<unsigned long long> ctr, per_mask;
    lk_key.alloc_exact((size_t)nslots);
    lk_slot.alloc_exact((size_t)nslots);
    ctr.alloc_exact(1, true, st);
    per_mask.alloc_exact((size_t)3 * M, true, st);
    hipLaunchKernelGGL(k_screen_prep, dim3(grid_for(nslots)), dim3(256), 0, st, v, d_kmers.p, d_rec_first.p, nslots, lk_key.p, lk_slot.p, ctr.p);
    HIPCHK(hipGetLastError());
    unsigned long long nlk_u = 0;
    HIPCHK(hipMemcpyAsync(&nlk_u, ctr.p, sizeof nlk_u, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int64_t nlk = (int64_t)nlk_u;
    out.stats.lookups += nlk;
    if (dbg) {
        std::vector<uint64_t> hk((size_t)nslots);
        HIPCHK(hipMemcpy(hk.data(), d_kmers.p, hk.size() * 8, hipMemcpyDeviceToHost));
        int64_t nz = 0;
        for (uint64_t x : hk) nz += x != 0;
        fprintf(stderr, "[lm] screen: %lld window records, %lld captured k-mers, %lld lookups\n", (long long)nrec, (long long)nz, (long long)nlk);
    }
    if (nlk == 0) {
        out.stats.ms_capture += t1 - t0;
        out.stats.ms_lookup += now_ms() - t1;
        return;
    }
    lk_key2.alloc_exact((size_t)nlk);
    lk_slot2.alloc_exact((size_t)nlk);
    prim_sort_pairs(st, tmp, lk_key.p, lk_key2.p, lk_slot.p, lk_slot2.p, (size_t)nlk, 0, SC_MASK_BITS + 1 + pb);
    lk_key.release();
    lk_slot.release();
    DBuf<int64_t> starts, offs;
    counts.alloc_exact((size_t)nlk + 1, true, st);
    starts.alloc_exact((size_t)nlk);
    offs.alloc_exact((size_t)nlk + 1);
    hipLaunchKernelGGL(k_screen_count, dim3(grid_for(nlk)), dim3(256), 0, st, v, d_kmers.p, lk_key2.p, lk_slot2.p, nlk, opt.min_prefix, counts.p,
                       starts.p, per_mask.p,
                       ix->sc_set ? ScreenShadowTab{ix->d_sc_bits.p, ix->d_sc_sum.p, ix->d_sc_kmers.p, ix->d_sc_off.p, ix->sc_W}
                                  : ScreenShadowTab{nullptr, nullptr, nullptr, nullptr, 0});
    HIPCHK(hipGetLastError());
    prim_scan_to_i64(st, tmp, counts.p, (size_t)nlk, offs.p);
    std::vector<uint64_t> pm((size_t)3 * M);
    HIPCHK(hipMemcpyAsync(pm.data(), per_mask.p, pm.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // ---- pieces of whole masks
    const int qbits = bits_for((int64_t)q1), gbits = bits_for(std::max<int64_t>(v.ngenomes, 2));
    const int qshift = SC_REC_SHIFT + gbits;
    if (qshift + qbits > 64)
        throw ArgError("lm_index_screen_genomes: " + std::to_string(q1) + " queries against " + std::to_string((long long)v.ngenomes) +
                        " records do not fit the 42 bits a tuple has for both: screen fewer queries per call");
    size_t fr = 0, tot = 0;
    HIPCHK(hipMemGetInfo(&fr, &tot));
    const int64_t per_tuple = 34 + 16; // (the arrays above, and the radix sort's scratch with room to spare)
    const int64_t hard = std::max<int64_t>(1024, ((int64_t)fr - ((int64_t)1 << 30)) / per_tuple);
    int64_t soft = std::min<int64_t>(hard, (int64_t)1 << 26);
    if (const char *e = getenv("LM_SCREEN_PIECE_TUPLES")) soft = std::min<int64_t>(hard, std::max<int64_t>(1, atoll(e)));
    std::vector<ScreenPiece> pieces;
    int bad = 0;
    if (!screen_pieces(pm.data(), M, soft, hard, pieces, &bad))
        throw DeviceOOM("lm_index_screen_genomes: mask " + std::to_string(bad) + " alone returns " + std::to_string((unsigned long long)pm[(size_t)bad]) +
                        " values for queries " + std::to_string(q0) + " .. " + std::to_string(q1 - 1) + "; at " + std::to_string((long long)per_tuple) +
                        " B each the tuples of one mask must fit the " + std::to_string(fr >> 20) + " MB free beside the index: screen fewer queries per call");
    std::vector<int64_t> lk_first((size_t)M + 1, 0), kept_first((size_t)M + 1, 0);
    for (int m = 0; m < M; m++) {
        lk_first[(size_t)m + 1] = lk_first[(size_t)m] + (int64_t)pm[(size_t)2 * M + m];
        kept_first[(size_t)m + 1] = kept_first[(size_t)m] + (int64_t)pm[(size_t)M + m];
    }
    if (lk_first.back() != nlk) throw HipError("lm_index_screen_genomes: the lookups counted per mask do not add up");
    const double t2 = now_ms();
    double t_emit = 0;
    DBuf<uint64_t> tk, tk2;
    DBuf<uint8_t> fm, frr, d_prefs;
    DBuf<int64_t> om, orr;
    DBuf<ScreenRowDev> d_rows;
    std::vector<ScreenRowDev> hrows;
    for (const ScreenPiece &P : pieces) {
        const double ta = now_ms();
        const int64_t j0 = lk_first[(size_t)P.m0], j1 = lk_first[(size_t)P.m1], n_all = P.tuples;
        const int64_t n = kept_first[(size_t)P.m1] - kept_first[(size_t)P.m0]; // the rest sorts behind them
        out.stats.pieces++;
        out.stats.tuples += n;
        try {
            tk.ensure((size_t)n_all);
            tk2.ensure((size_t)n_all);
            fm.ensure((size_t)n + 1);
            frr.ensure((size_t)n + 1);
            om.ensure((size_t)n + 1);
            orr.ensure((size_t)n + 1);
        } catch (const DeviceOOM &e) {
            throw DeviceOOM("lm_index_screen_genomes: the " + std::to_string((long long)n_all) + " tuples of masks " + std::to_string(P.m0) + " .. " +
                            std::to_string(P.m1 - 1) + " need 34 B each on the device beside the index: " + e.what());
        }
        hipLaunchKernelGGL(k_screen_emit, dim3(grid_for(j1 - j0)), dim3(256), 0, st, v, d_kmers.p, d_rec2q.p, lk_key2.p, lk_slot2.p, j0, j1, counts.p,
                           offs.p, starts.p, qshift, tk.p);
        HIPCHK(hipGetLastError());
        if (dbg) HIPCHK(hipStreamSynchronize(st));
        const double tb = now_ms();
        t_emit += tb - ta;
        if (n == 0) continue;
        prim_sort_keys(st, tmp, tk.p, tk2.p, (size_t)n_all, 0, std::min(64, qshift + qbits));
        hipLaunchKernelGGL(k_screen_flags, dim3(grid_for(n + 1)), dim3(256), 0, st, tk2.p, n, fm.p, frr.p);
        HIPCHK(hipGetLastError());
        prim_scan_to_i64(st, tmp, fm.p, (size_t)n, om.p);
        prim_scan_to_i64(st, tmp, frr.p, (size_t)n, orr.p);
        int64_t ngm = 0, ngr = 0;
        HIPCHK(hipMemcpyAsync(&ngm, om.p + n, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&ngr, orr.p + n, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        d_rows.ensure((size_t)ngr);
        HIPCHK(hipMemsetAsync(d_rows.p, 0, (size_t)ngr * sizeof(ScreenRowDev), st));
        if (opt.details) d_prefs.ensure((size_t)ngm);
        hipLaunchKernelGGL(k_screen_reduce, dim3(grid_for((n + SC_RUN - 1) / SC_RUN)), dim3(256), 0, st, tk2.p, n, fm.p, frr.p, om.p, orr.p, d_rows.p,
                           opt.details ? d_prefs.p : nullptr);
        HIPCHK(hipGetLastError());
        hrows.resize((size_t)ngr);
        HIPCHK(hipMemcpyAsync(hrows.data(), d_rows.p, (size_t)ngr * sizeof(ScreenRowDev), hipMemcpyDeviceToHost, st));
        const size_t pref_base = out.prefs.size();
        if (opt.details) {
            out.prefs.resize(pref_base + (size_t)ngm);
            HIPCHK(hipMemcpyAsync(out.prefs.data() + pref_base, d_prefs.p, (size_t)ngm, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        for (const ScreenRowDev &r : hrows) {
            ScreenPartial p;
            p.query = (uint32_t)(r.key >> gbits);
            p.local = (int64_t)(r.key & (((uint64_t)1 << gbits) - 1));
            p.score = r.score;
            p.score2 = r.score2;
            p.hit_kmers = r.hit_kmers;
            p.hit_masks = r.hit_masks;
            p.pref_off = pref_base + r.pref_first;
            out.partials.push_back(p);
        }
        out.stats.ms_reduce += now_ms() - tb;
    }
    out.stats.ms_capture += t1 - t0;
    out.stats.ms_lookup += (t2 - t1) + t_emit;
}

} // namespace lm

struct lm_screen {
    std::vector<lm_screen_row> rows;
    std::vector<uint64_t> keys;
    std::vector<uint8_t> prefixes;
    lm_screen_stats stats;
};

extern "C" void lm_screen_opt_default(lm_screen_opt *o) {
    if (!o) return;
    o->min_prefix = 21;
    o->windows = 1;
    o->top_n = 10;
    o->details = 0;
}

extern "C" lm_status lm_index_screen_genomes(lm_index *ix, const lm_genome_query *queries, size_t nq, const lm_screen_opt *opt_in, lm_screen **out) {
    using namespace lm;
    if (!ix || !out) return LM_ERR_ARG;
    *out = nullptr;
    lm_screen_opt opt;
    lm_screen_opt_default(&opt);
    if (opt_in) opt = *opt_in;
    std::unique_ptr<lm_screen> res(new lm_screen());
    memset(&res->stats, 0, sizeof res->stats);
    const lm_status rc = guarded(ix, "lm_index_screen_genomes: the host could not hold the batch or its rows", [&]() {
        const HostIndex &h = ix->host;
        const double t0 = now_ms();
        if (opt.windows < 1) throw ArgError("lm_index_screen_genomes: windows = " + std::to_string(opt.windows) + ", needs to be > 0");
        if (opt.top_n < 0) throw ArgError("lm_index_screen_genomes: top_n = " + std::to_string(opt.top_n) + " is negative");
        if (opt.min_prefix > h.k || opt.min_prefix < h.mask_prefix + h.anchor_prefix)
            throw OptionError("lm_index_screen_genomes: min_prefix (" + std::to_string(opt.min_prefix) + ") should be in the range of [" +
                               std::to_string(h.mask_prefix + h.anchor_prefix) + ", " + std::to_string(h.k) + "]");
        if (nq > 0 && !queries) throw ArgError("lm_index_screen_genomes: queries is NULL but nq is not 0");
        if (nq >= ((size_t)1 << 31)) throw ArgError("lm_index_screen_genomes: more than 2^31 queries");
        std::vector<ScreenLayout> lay(nq);
        for (size_t q = 0; q < nq; q++) {
            const std::string name = "query " + std::to_string(q) + (queries[q].id ? std::string(" (") + queries[q].id + ")" : std::string());
            if (queries[q].ncontigs == 0 || !queries[q].contigs) throw ArgError("lm_index_screen_genomes: " + name + " has no contigs");
            std::vector<uint32_t> cl(queries[q].ncontigs);
            for (size_t c = 0; c < cl.size(); c++) {
                cl[c] = queries[q].contigs[c].len;
                if (cl[c] && !queries[q].contigs[c].seq) throw ArgError("lm_index_screen_genomes: contig " + std::to_string(c) + " of " + name + " has no sequence");
            }
            screen_layout(cl.data(), cl.size(), h.k, lay[q]);
            if (lay[q].len >= ((int64_t)1 << 28))
                throw ArgError("lm_index_screen_genomes: " + name + " has " + std::to_string((long long)lay[q].len) +
                                " bases with its spacers; a query genome must stay below 2^28");
        }
        // sub-batches: window records x masks stay below 2^30 lookup slots, the concatenations below 2^30 bytes
        ScreenOut so;
        memset(&so.stats, 0, sizeof so.stats);
        for (size_t q0 = 0; q0 < nq;) {
            size_t q1 = q0;
            int64_t slots = 0, bases = 0;
            while (q1 < nq) {
                const int64_t s = (int64_t)opt.windows * h.M, b = lay[q1].len;
                if (q1 > q0 && (slots + s > ((int64_t)1 << 30) || bases + b > ((int64_t)1 << 30))) break;
                slots += s;
                bases += b;
                q1++;
            }
            if (slots >= ((int64_t)1 << 32)) throw ArgError("lm_index_screen_genomes: windows x masks of one query must stay below 2^32");
            screen_sub_batch(ix, queries, lay, q0, q1, opt, so);
            q0 = q1;
        }
        ix->lane[0].main.tmp.release();
        // ---- rows
        std::vector<ScreenPartial> recs;
        std::vector<std::vector<size_t>> chain;
        screen_merge_partials(so.partials, recs, chain);
        std::vector<ScreenHit> hits(recs.size());
        for (size_t i = 0; i < recs.size(); i++) {
            if (recs[i].local < 0 || recs[i].local >= (int64_t)h.genomes.size()) throw HipError("lm_index_screen_genomes: a tuple names a record the handle does not hold");
            const uint64_t key = h.genomes[(size_t)recs[i].local].bg;
            const auto it = h.chunk_of.find(key);
            hits[i] = ScreenHit{recs[i].query, key, it == h.chunk_of.end() ? -1 : (int32_t)it->second.list, recs[i].score};
        }
        std::vector<ScreenRow> rows;
        screen_rows(hits, opt.top_n, rows);
        std::vector<uint64_t> first_key(rows.size());
        for (size_t i = 0; i < rows.size(); i++) first_key[i] = rows[i].keys[0];
        std::vector<const char *> names;
        genome_ids_of_keys(ix, first_key, names);
        for (size_t i = 0; i < rows.size(); i++) {
            const ScreenRow &r = rows[i];
            const ScreenPartial &d = recs[r.detail];
            lm_screen_row o;
            memset(&o, 0, sizeof o);
            o.query = r.query;
            o.nkeys = (uint32_t)r.keys.size();
            o.score = r.score;
            o.batch_genome = r.keys[0];
            o.genome_id = names[i];
            o.keys_off = res->keys.size();
            res->keys.insert(res->keys.end(), r.keys.begin(), r.keys.end());
            o.prefixes_off = res->prefixes.size();
            if (opt.details) {
                o.score2 = d.score2;
                o.hit_masks = d.hit_masks;
                o.hit_kmers = d.hit_kmers;
                for (size_t pi : chain[r.detail]) {
                    const ScreenPartial &p = so.partials[pi];
                    res->prefixes.insert(res->prefixes.end(), so.prefs.begin() + (std::ptrdiff_t)p.pref_off,
                                         so.prefs.begin() + (std::ptrdiff_t)(p.pref_off + p.hit_masks));
                }
                std::sort(res->prefixes.begin() + (std::ptrdiff_t)o.prefixes_off, res->prefixes.end(), [](uint8_t a, uint8_t b) { return a > b; });
            }
            res->rows.push_back(o);
        }
        res->stats = so.stats;
        res->stats.ms_total = now_ms() - t0;
    });
    if (rc == LM_OK) *out = res.release();
    return rc;
}


// ---- the list structure of a shard (ScreenShadowTab, lm_kernels.h).  Blob: magic, K, M, mask prefix, anchor bases, W, outlier count;
// bits [2M * W]; off [2M + 1]; k-mers.
namespace lm {
static const uint64_t SC_BLOB_MAGIC = 0x314254534d4c; // "LMSTB1"
struct ScreenBlobHead {
    uint64_t magic;
    int32_t K, M, p, a, W, pad;
    int64_t nout;
};
static void screen_local_structure(lm_index *ix, std::vector<uint64_t> &bits, std::vector<int64_t> &off, std::vector<uint64_t> &kmers, int &W) {
    const hipStream_t st = ix->lane[0].main.st;
    const DevIndexView &v = ix->view;
    W = (v.P1 - 1 + 63) / 64;
    if (W > 64) throw ArgError("screen structure: a partition index of more than 6 bases is not supported");
    const size_t nb = (size_t)2 * v.M * W;
    DBuf<uint64_t> d;
    d.alloc_exact(nb);
    hipLaunchKernelGGL(k_screen_occupancy, dim3(grid_for((int64_t)nb)), dim3(256), 0, st, v, W, d.p);
    HIPCHK(hipGetLastError());
    bits.resize(nb);
    off.resize((size_t)2 * v.M + 1);
    HIPCHK(hipMemcpyAsync(bits.data(), d.p, nb * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(off.data(), ix->d_out_off.p, off.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    kmers.resize((size_t)off.back());
    if (!kmers.empty()) HIPCHK(hipMemcpyAsync(kmers.data(), ix->d_out_kmers.p, kmers.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}
} // namespace lm

static const char *const SC_STRUCTURE_NOMEM = "screen structure: the host could not hold it"; // (neither call throws an OptionError)

extern "C" lm_status lm_index_screen_structure(lm_index *ix, void **blob, size_t *bytes) {
    using namespace lm;
    if (!ix || !blob || !bytes) return LM_ERR_ARG;
    *blob = nullptr;
    *bytes = 0;
    return guarded(ix, SC_STRUCTURE_NOMEM, [&]() {
        std::vector<uint64_t> bits, kmers;
        std::vector<int64_t> off;
        int W = 0;
        screen_local_structure(ix, bits, off, kmers, W);
        const HostIndex &h = ix->host;
        ScreenBlobHead hd{SC_BLOB_MAGIC, h.k, h.M, h.mask_prefix, ix->view.part_bases, W, 0, (int64_t)kmers.size()};
        const size_t n = sizeof hd + bits.size() * 8 + off.size() * 8 + kmers.size() * 8;
        char *p = (char *)malloc(n);
        if (!p) throw std::bad_alloc();
        memcpy(p, &hd, sizeof hd);
        memcpy(p + sizeof hd, bits.data(), bits.size() * 8);
        memcpy(p + sizeof hd + bits.size() * 8, off.data(), off.size() * 8);
        if (!kmers.empty()) memcpy(p + sizeof hd + bits.size() * 8 + off.size() * 8, kmers.data(), kmers.size() * 8);
        *blob = p;
        *bytes = n;
    });
}

extern "C" lm_status lm_index_screen_add_structure(lm_index *ix, const void *blob, size_t bytes) {
    using namespace lm;
    if (!ix) return LM_ERR_ARG;
    return guarded(ix, SC_STRUCTURE_NOMEM, [&]() {
        if (!blob || bytes == 0) { // back to the handle's own lists
            ix->sc_set = false;
            return;
        }
        const hipStream_t st = ix->lane[0].main.st;
        const HostIndex &h = ix->host;
        ScreenBlobHead hd;
        if (bytes < sizeof hd) throw ArgError("lm_index_screen_add_structure: the blob is shorter than its header");
        memcpy(&hd, blob, sizeof hd);
        const int Wl = (ix->view.P1 - 1 + 63) / 64;
        if (hd.magic != SC_BLOB_MAGIC) throw ArgError("lm_index_screen_add_structure: not a structure of lm_index_screen_structure");
        if (hd.K != h.k || hd.M != h.M || hd.p != h.mask_prefix || hd.a != ix->view.part_bases || hd.W != Wl)
            throw ArgError("lm_index_screen_add_structure: the structure is of an index with other k, masks or partitions (k " + std::to_string(hd.K) +
                            ", " + std::to_string(hd.M) + " masks, " + std::to_string(hd.a) + " partition bases)");
        const size_t nb = (size_t)2 * h.M * Wl, no = (size_t)2 * h.M + 1;
        if (hd.nout < 0 || bytes != sizeof hd + nb * 8 + no * 8 + (size_t)hd.nout * 8)
            throw ArgError("lm_index_screen_add_structure: the blob's length does not fit its header");
        // (a caller's buffer need not be aligned: the three arrays are copied out)
        std::vector<uint64_t> fb(nb), fk((size_t)hd.nout);
        std::vector<int64_t> fo(no);
        const char *src = (const char *)blob + sizeof hd;
        memcpy(fb.data(), src, nb * 8);
        memcpy(fo.data(), src + nb * 8, no * 8);
        if (hd.nout) memcpy(fk.data(), src + nb * 8 + no * 8, (size_t)hd.nout * 8);
        if (fo[0] != 0 || fo[no - 1] != hd.nout) throw ArgError("lm_index_screen_add_structure: the blob's outlier table is broken");
        for (size_t i = 0; i + 1 < no; i++) {
            if (fo[i + 1] < fo[i]) throw ArgError("lm_index_screen_add_structure: the blob's outlier table is broken");
            if (!std::is_sorted(fk.begin() + fo[i], fk.begin() + fo[i + 1]))
                throw ArgError("lm_index_screen_add_structure: the outlier k-mers of list " + std::to_string(i) + " of the blob are not ascending");
        }
        // the union is made beside what the handle holds and takes its place only when it is whole, on the host and on the
        // device; a failure on the way leaves the handle with its own lists (sc_set = false), never with half of a union
        std::vector<uint64_t> bits, kmers;
        std::vector<int64_t> off;
        if (ix->sc_set) {
            bits = ix->sc_bits;
            kmers = ix->sc_kmers;
            off = ix->sc_off;
        } else {
            int W = 0;
            screen_local_structure(ix, bits, off, kmers, W);
        }
        for (size_t i = 0; i < nb; i++) bits[i] |= fb[i];
        std::vector<uint64_t> mk;
        std::vector<int64_t> mo(no, 0);
        mk.reserve(kmers.size() + (size_t)hd.nout);
        for (size_t md = 0; md + 1 < no; md++) { // per list: both ascending
            std::merge(kmers.begin() + off[md], kmers.begin() + off[md + 1], fk.begin() + fo[md], fk.begin() + fo[md + 1], std::back_inserter(mk));
            mo[md + 1] = (int64_t)mk.size();
        }
        std::vector<uint64_t> sum((size_t)2 * h.M, 0);
        for (size_t md = 0; md < sum.size(); md++)
            for (int w = 0; w < Wl; w++)
                if (bits[md * Wl + w]) sum[md] |= 1ull << w;
        ix->sc_set = false;
        ix->d_sc_bits.alloc_exact(nb);
        ix->d_sc_sum.alloc_exact(sum.size());
        ix->d_sc_off.alloc_exact(no);
        ix->d_sc_kmers.alloc_exact(std::max<size_t>(mk.size(), 1));
        HIPCHK(hipMemcpyAsync(ix->d_sc_bits.p, bits.data(), nb * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ix->d_sc_sum.p, sum.data(), sum.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ix->d_sc_off.p, mo.data(), no * 8, hipMemcpyHostToDevice, st));
        if (!mk.empty()) HIPCHK(hipMemcpyAsync(ix->d_sc_kmers.p, mk.data(), mk.size() * 8, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        ix->sc_bits = std::move(bits);
        ix->sc_kmers = std::move(mk);
        ix->sc_off = std::move(mo);
        ix->sc_W = Wl;
        ix->sc_set = true;
    });
}

extern "C" size_t lm_screen_rows(const lm_screen *s, const lm_screen_row **rows) {
    if (!s) return 0;
    if (rows) *rows = s->rows.data();
    return s->rows.size();
}
extern "C" size_t lm_screen_keys(const lm_screen *s, const uint64_t **keys) {
    if (!s) return 0;
    if (keys) *keys = s->keys.data();
    return s->keys.size();
}
extern "C" size_t lm_screen_prefixes(const lm_screen *s, const uint8_t **prefixes) {
    if (!s) return 0;
    if (prefixes) *prefixes = s->prefixes.data();
    return s->prefixes.size();
}
extern "C" void lm_screen_get_stats(const lm_screen *s, lm_screen_stats *stats) {
    if (s && stats) *stats = s->stats;
}
extern "C" void lm_screen_free(lm_screen *s) { delete s; }

// search-genome.go:577-590
extern "C" int lm_format_screen_row(const lm_screen_row *row, const uint8_t *prefixes, const char *query_id, int min_prefix, int masks, int extra,
                                    char *buf, size_t buflen) {
    if (!row) return 0;
    std::string line;
    char head[160];
    const double frac = (double)row->hit_masks / (double)masks, avg = (double)row->score2 / (double)row->hit_masks;
    char avg_s[48];
    if (std::isnan(avg)) snprintf(avg_s, sizeof avg_s, "NaN"); // (Go's %.2f of 0 / 0: a row without details)
    else snprintf(avg_s, sizeof avg_s, "%.2f", avg);
    snprintf(head, sizeof head, "\t%d\t%.4f\t%u\t%llu\t%s", min_prefix, frac, row->hit_masks, (unsigned long long)row->score2, avg_s);
    line = std::string(query_id ? query_id : "") + "\t" + (row->genome_id ? row->genome_id : "") + head;
    if (extra) {
        line += "\t";
        for (uint32_t i = 0; prefixes && i < row->hit_masks; i++) {
            if (i) line += ",";
            line += std::to_string((int)prefixes[row->prefixes_off + i]);
        }
    }
    if (buf && buflen) {
        const size_t n = std::min(line.size(), buflen - 1);
        memcpy(buf, line.data(), n);
        buf[n] = 0;
    }
    return (int)line.size();
}
// search-genome.go:482-486
extern "C" const char *lm_screen_header(int extra) {
    return extra ? "query\tsubject\tminPrefix\tfracMasks\tnMasks\tsumPrefix\tavgPrefix\tprefixes"
                 : "query\tsubject\tminPrefix\tfracMasks\tnMasks\tsumPrefix\tavgPrefix";
}
