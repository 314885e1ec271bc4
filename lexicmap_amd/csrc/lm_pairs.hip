// lm_pairs.hip — similar genome pairs of a resident index on the device: lm_index_genome_pairs (include/lexicmap_hip.h;
// DESIGN.md section 11).  What `lexicmap genome pair -s 0` computes (lexicmap/cmd/pair.go), from the packed image alone.
//
//   k_pair_entries   the forward seeds of the selected masks - per mask the packed list md = 2 m, then its flat outliers - in
//                    list order, as (k-mer, record slot, mask in selection); seeds of records outside the selection are left
//                    out.  Two passes over tiles of 256 seeds: COUNT writes the kept seeds per tile, after a scan of those
//                    numbers WRITE places a seed at tile offset + wavefront offset + rank among the kept lanes.
//   k_pair_heads     an entry opens a group when it is the first of its mask or differs from its predecessor in the top
//                    min_prefix bases (min_prefix >= mask prefix + partition bases: a group lies inside one partition, or inside
//                    the outlier list, where k-mers ascend); an inclusive max-scan of the head positions gives every entry
//                    its group's head, k_pair_counts its candidate tuples j - head(j): one per earlier entry of the group.
//   pieces           an exclusive scan of those counts numbers the tuples; the host cuts the masks into pieces of whole
//                    masks whose tuples fit the device and whose key fits 64 bits (lm_pair_plan.h); per piece:
//   k_pair_emit      the lanes over the flat TUPLE index: a lane finds its entry by binary search in the scan (between the
//                    brackets its tile found once), its partner by offset, and writes slot1 | slot2 | mask in piece | LCP;
//                    two seeds of one record write the all-ones key, which sorts behind the rest.
//   radix sort       over the used bits; k_pair_flags + one scan number the pairs,
//   k_pair_reduce    a lane walks 16 sorted tuples: the last key of a (pair, mask) run holds the largest LCP (it sits in the
//                    lowest bits) and adds (1, LCP) to its pair, one atomic per row change of the lane.
//   accumulate       the piece's partial rows behind the table, one radix sort by pair, k_pair_merge_flags adds the (at most
//                    two) entries of a pair and applies the exact prune, a scan and k_pair_merge_scatter compact the table.
//                    The table stays on the device; after the last piece the prune is the filter by `required`.
//   finish           one stable radix sort by ~(n_masks << 32 | sum_prefix) of the table (ascending by pair) is the rule's
//                    order; the host maps slots to keys and names.
// Memory: 36 B per entry while the heads are scanned, 28 B afterwards; 25 B per tuple of a piece and 32 B per table row,
// each plus the radix sort's scratch.
//
// Across shards (lm_index_pair_seeds, lm_index_genome_pairs_across, lm_pairs_merge; host part lm_pair_cross_plan.h): a rank
// exports its entries as a blob; the rank that receives blobs puts their entries behind its own (k_pair_pack_own /
// k_pair_pack_blob), sorts all of them stably by the top min_prefix bases and then by mask - a group's own entries stay ahead
// of its blob entries - and counts per entry the OWN entries ahead of it in its group (k_pair_unpack, a scan of the own
// flags, k_pair_counts_two); k_pair_emit<true> finds the partner at head + offset.  From the pieces on the passes are the
// same.  32 B per entry while sorted, 49 B while the groups are scanned, 32 B afterwards.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <deque>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "lm_internal.h"
#include "lm_lookup_dev.h"
#include "lm_merge.h"
#include "lm_pair_cross_plan.h"
#include "lm_pair_plan.h"
#include "lm_prims.h"
#include "lm_seed_walk.h"

namespace lm {

#define PR_RUN 16 /* sorted tuples per lane of k_pair_reduce */

__device__ __forceinline__ int pr_lane_rank(unsigned long long bal) { // kept lanes below this one (mbcnt)
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

struct PairEntArgs {
    const int32_t *sel_mask; // [ns] the selected masks
    const int64_t *eoff;     // [ns + 1] first raw entry of every selected mask: packed forward seeds, then forward outliers
    int32_t ns;
    int64_t nraw, ntiles;
    const int32_t *slot_of_local; // [nlocal] slot of a record in the selection, -1: not selected
    int64_t nlocal;
    uint32_t *tile_cnt;      // [ntiles + 1] (COUNT writes it; the last stays 0)
    const int64_t *tile_off; // its exclusive scan (WRITE reads it)
    uint64_t *e_kmer;        // [n]
    uint32_t *e_slot, *e_ms; // [n]
    int64_t cap;
};

template <bool COUNT> __global__ __launch_bounds__(256) void k_pair_entries(DevIndexView ix, PairEntArgs a) {
    __shared__ uint32_t wcnt[4];
    const int lane = (int)(threadIdx.x & 63u), w = (int)(threadIdx.x >> 6);
    const int P = ix.P1 - 1;
    const int val_bits = ix.gid_bits + ix.pos_bits + 1;
    for (int64_t ti = blockIdx.x; ti < a.ntiles; ti += gridDim.x) {
        const int64_t t0 = ti * 256, t1 = (t0 + 256 < a.nraw ? t0 + 256 : a.nraw) - 1;
        int64_t lf, ll;
        sw_tile_lists(a.eoff, 0, (int64_t)a.ns, t0, t1, &lf, &ll);
        const int64_t i = t0 + threadIdx.x;
        int32_t slot = -1;
        uint64_t kmer = 0;
        int64_t s = 0;
        if (i <= t1) {
            s = sw_last_le(a.eoff, lf, ll, i);
            const int64_t m = a.sel_mask[s], md = 2 * m, rel = i - a.eoff[s];
            const int64_t base = ix.md_off[md], npk = ix.md_off[md + 1] - base;
            if (rel < npk) {
                const uint64_t pv = lm_bits_get(ix.pk_vals, base + rel, val_bits);
                const uint64_t local = lm_packed_val_genome(pv, ix.pos_bits);
                if ((int64_t)local < a.nlocal) slot = a.slot_of_local[local];
                if (!COUNT && slot >= 0) {
                    const int part = (int)sw_last_le(ix.part_tab + md * ix.P1, 0, P - 1, rel);
                    const uint64_t pfx = ix.masks[m] >> ((ix.K - ix.mask_prefix) << 1);
                    kmer = (((pfx << (ix.part_bases << 1)) | (uint64_t)part) << ix.key_bits) | lm_bits_get(ix.pk_keys, base + rel, ix.key_bits);
                }
            } else {
                const int64_t o = ix.out_off[md] + (rel - npk);
                const int g = local_genome(ix, ix.out_vals[o] >> 30);
                if (g >= 0 && (int64_t)g < a.nlocal) slot = a.slot_of_local[g];
                if (!COUNT) kmer = ix.out_kmers[o];
            }
        }
        const bool kept = slot >= 0;
        const unsigned long long bal = __ballot(kept);
        if (lane == 0) wcnt[w] = (uint32_t)__popcll(bal);
        __syncthreads();
        if (COUNT) {
            if (threadIdx.x == 0) a.tile_cnt[ti] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        } else if (kept) {
            int64_t o = a.tile_off[ti] + pr_lane_rank(bal);
            for (int x = 0; x < w; x++) o += wcnt[x];
            if (o < a.cap) {
                a.e_kmer[o] = kmer;
                a.e_slot[o] = (uint32_t)slot;
                a.e_ms[o] = (uint32_t)s;
            }
        }
        __syncthreads(); // (wcnt is written again by the next tile)
    }
}

// hp[j] = j where entry j opens a group, else 0: its inclusive max-scan is the head of every entry's group
__global__ void k_pair_heads(const uint64_t *__restrict__ kmer, const uint32_t *__restrict__ ms, int64_t n, int shift, int64_t *__restrict__ hp) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const bool head = j == 0 || ms[j] != ms[j - 1] || (kmer[j] >> shift) != (kmer[j - 1] >> shift);
    hp[j] = head ? j : 0;
}
// cnt[j] = j - head(j): the candidate tuples of entry j; cnt[n] = 0 (the scan's total)
__global__ void k_pair_counts(const int64_t *__restrict__ head, int64_t n, uint32_t *__restrict__ cnt) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    cnt[j] = j < n ? (uint32_t)(j - head[j]) : 0u;
}
// ceoff[s] = the first entry of selected mask s (a mask without entries starts where the next one does), ceoff[ns] = n
__global__ void k_pair_mask_bounds(const uint32_t *__restrict__ ms, int64_t n, int32_t ns, int64_t *__restrict__ ceoff) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e > n) return;
    const int64_t hi = e < n ? (int64_t)ms[e] : (int64_t)ns;
    const int64_t lo = e > 0 ? (int64_t)ms[e - 1] + 1 : 0;
    for (int64_t s = lo; s <= hi && s <= (int64_t)ns; s++) ceoff[s] = e;
}
__global__ void k_pair_mask_totals(const int64_t *__restrict__ ceoff, const int64_t *__restrict__ offs, int32_t ns, int64_t *__restrict__ tot) {
    const int32_t s = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s < ns) tot[s] = offs[ceoff[s + 1]] - offs[ceoff[s]];
}

// ---- the two-sided form (lm_index_genome_pairs_across): own entries and the entries of other shards' blobs in one array.
// While they are sorted an entry travels as its k-mer and pk = mask in selection << 32 | blob << 31 | slot (slots < 2^29).
#define PR_BLOB_BIT 0x80000000u
__global__ void k_pair_pack_own(const uint32_t *__restrict__ slot, const uint32_t *__restrict__ ms, int64_t n, uint64_t *__restrict__ pk) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) pk[j] = ((uint64_t)ms[j] << 32) | slot[j];
}
// a blob's entries: rec[i] indexes the blob's records, whose slots in the union are slot_of_rec [nrec]; eoff [ns + 1] is the
// blob's first entry of every selected mask
__global__ void k_pair_pack_blob(const uint32_t *__restrict__ rec, int64_t n, const int64_t *__restrict__ eoff, int32_t ns,
                                 const uint32_t *__restrict__ slot_of_rec, int64_t nrec, uint64_t *__restrict__ pk) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = (uint64_t)sw_last_le(eoff, 0, (int64_t)ns - 1, i);
    const uint32_t r = rec[i];
    pk[i] = (s << 32) | PR_BLOB_BIT | ((int64_t)r < nrec ? slot_of_rec[r] : 0u); // (the host refused a blob with r >= nrec)
}
// own[j] = entry j is an own one; own[n] = 0 (the scan's total)
__global__ void k_pair_unpack(const uint64_t *__restrict__ pk, int64_t n, uint32_t *__restrict__ slot, uint32_t *__restrict__ ms,
                              uint8_t *__restrict__ own) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) {
        own[j] = 0;
        return;
    }
    const uint64_t v = pk[j];
    slot[j] = (uint32_t)v & (PR_BLOB_BIT - 1u);
    ms[j] = (uint32_t)(v >> 32);
    own[j] = ((uint32_t)v & PR_BLOB_BIT) == 0;
}
// ownx: the exclusive scan of own.  A group's own entries come first, so the own entries ahead of j in its group,
// ownx[j] - ownx[head(j)], are j - head(j) for an own entry and the group's own-count for a blob entry: the candidates of
// j, which lie at head(j) + t.  back[j] = j - head(j); cnt[n] = 0.
__global__ void k_pair_counts_two(const int64_t *__restrict__ head, const int64_t *__restrict__ ownx, int64_t n, uint32_t *__restrict__ cnt,
                                  uint32_t *__restrict__ back) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) {
        cnt[j] = 0;
        return;
    }
    const int64_t h = head[j];
    cnt[j] = (uint32_t)(ownx[j] - ownx[h]);
    back[j] = (uint32_t)(j - h);
}

// The tuples [0, n) of a piece: tuple t is number tbase + t of the scan `offs` and belongs to the entries [e0, e1) of the
// piece's masks [s0, ..).  One tuple per lane, so a group of any size is shared by as many wavefronts as its tuples fill.
// TWO (lm_index_genome_pairs_across with blob entries): a group's own entries lie ahead of its blob entries and an entry's
// candidates are the OWN entries ahead of it, so cnt[j] is no longer j - head(j): back[j] holds that distance.
template <bool TWO>
__global__ __launch_bounds__(256) void k_pair_emit(const uint64_t *__restrict__ kmer, const uint32_t *__restrict__ slot,
                                                   const uint32_t *__restrict__ ms, const uint32_t *__restrict__ cnt,
                                                   const uint32_t *__restrict__ back, const int64_t *__restrict__ offs, int64_t e0, int64_t e1,
                                                   int64_t tbase, int64_t n, uint32_t s0, int K, int slot_bits, int mask_bits,
                                                   uint64_t *__restrict__ out) {
    for (int64_t t0 = (int64_t)blockIdx.x * blockDim.x; t0 < n; t0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t1 = (t0 + (int64_t)blockDim.x < n ? t0 + (int64_t)blockDim.x : n) - 1;
        int64_t jf, jl;
        sw_tile_lists(offs, e0, e1, tbase + t0, tbase + t1, &jf, &jl);
        const int64_t t = t0 + threadIdx.x;
        if (t > t1) continue;
        const int64_t T = tbase + t;
        const int64_t j = sw_last_le(offs, jf, jl, T); // the last entry that starts at or before T: it has tuples, T is one of them
        const int64_t i = j - (int64_t)(TWO ? back[j] : cnt[j]) + (T - offs[j]);
        const uint32_t a = slot[i], b = slot[j];
        uint64_t key = ~0ull;
        if (a != b) {
            const uint64_t x = kmer[i], y = kmer[j];
            const int lcp = x == y ? K : lm_lcp(x, y, K);
            const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
            key = (((lo << slot_bits) | hi) << (mask_bits + LM_PAIR_LEN_BITS)) | ((uint64_t)(ms[j] - s0) << LM_PAIR_LEN_BITS) | (uint64_t)lcp;
        }
        out[t] = key;
    }
}

// fr[i]: sorted tuple i opens a pair.  n + 1 entries, the last 0 (the scan's total).  All-ones keys (same record) open nothing.
__global__ void k_pair_flags(const uint64_t *__restrict__ keys, int64_t n, int pair_shift, uint8_t *__restrict__ fr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        fr[i] = 0;
        return;
    }
    const uint64_t k = keys[i];
    fr[i] = k != ~0ull && (i == 0 || (k >> pair_shift) != (keys[i - 1] >> pair_shift));
}

// orr: exclusive scan of fr.  rows_pair / rows_val (zeroed) [orr[n]]: pair, n_masks << 32 | sum_prefix
__global__ __launch_bounds__(256) void k_pair_reduce(const uint64_t *__restrict__ keys, int64_t n, int pair_shift, const uint8_t *__restrict__ fr,
                                                     const int64_t *__restrict__ orr, uint64_t *__restrict__ rows_pair,
                                                     unsigned long long *__restrict__ rows_val) {
    const int64_t i0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * PR_RUN;
    if (i0 >= n) return;
    const int64_t i1 = i0 + PR_RUN < n ? i0 + PR_RUN : n;
    int64_t row = orr[i0] + fr[i0] - 1;
    unsigned long long acc = 0;
    for (int64_t i = i0; i < i1; i++) {
        const uint64_t k = keys[i];
        if (k == ~0ull) break; // (they sort behind every tuple of two records)
        if (fr[i]) {
            if (i > i0) {
                if (acc) atomicAdd(&rows_val[row], acc);
                acc = 0;
                row++;
            }
            rows_pair[row] = k >> pair_shift;
        }
        // the last tuple of a (pair, mask) run: the largest LCP of the mask
        if (i + 1 == n || (keys[i + 1] >> LM_PAIR_LEN_BITS) != (k >> LM_PAIR_LEN_BITS)) acc += (1ull << 32) | (k & ((1ull << LM_PAIR_LEN_BITS) - 1));
    }
    if (acc) atomicAdd(&rows_val[row], acc);
}

// table and partial rows sorted by pair together: a pair is there once or twice.  fh[i]: entry i is the first of its pair;
// fk[i]: and the pair stays (n_masks so far + masks_left >= required).  n + 1 entries, the last 0.
__global__ void k_pair_merge_flags(const uint64_t *__restrict__ pair, const unsigned long long *__restrict__ val, int64_t n, int64_t masks_left,
                                   int64_t required, uint8_t *__restrict__ fh, uint8_t *__restrict__ fk) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        fh[i] = fk[i] = 0;
        return;
    }
    const uint64_t p = pair[i];
    const bool head = i == 0 || pair[i - 1] != p;
    unsigned long long v = val[i];
    if (head && i + 1 < n && pair[i + 1] == p) v += val[i + 1];
    fh[i] = head;
    fk[i] = head && (int64_t)(v >> 32) + masks_left >= required;
}
__global__ void k_pair_merge_scatter(const uint64_t *__restrict__ pair, const unsigned long long *__restrict__ val, int64_t n,
                                     const uint8_t *__restrict__ fk, const int64_t *__restrict__ pos, uint64_t *__restrict__ out_pair,
                                     unsigned long long *__restrict__ out_val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !fk[i]) return;
    unsigned long long v = val[i];
    if (i + 1 < n && pair[i + 1] == pair[i]) v += val[i + 1];
    out_pair[pos[i]] = pair[i];
    out_val[pos[i]] = v;
}
// the order key of a row: ascending ~(n_masks << 32 | sum_prefix) is n_masks descending, then sum_prefix descending
__global__ void k_pair_order_keys(const unsigned long long *__restrict__ val, int64_t n, uint64_t *__restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = ~(uint64_t)val[i];
}

static void pr_max_scan(hipStream_t st, DBuf<uint8_t> &tmp, int64_t *io, size_t n) {
    if (n == 0) return;
    size_t bytes = 0;
    RPCHK(rocprim::inclusive_scan(nullptr, bytes, io, io, n, rocprim::maximum<int64_t>(), st));
    tmp.ensure(bytes);
    RPCHK(rocprim::inclusive_scan(tmp.p, bytes, io, io, n, rocprim::maximum<int64_t>(), st));
}

struct PairOut {
    std::vector<PairRow> rows; // in the rule's order; pair = slot1 << 32 | slot2 here
    std::vector<uint64_t> slot_key;
    std::vector<int32_t> slot_src; // -1: an own record, else the blob that holds the record (empty: all own)
    std::vector<int64_t> slot_idx; // ... and its number there
    lm_pair_stats stats;
};
// the parsed blobs of lm_index_genome_pairs_across (their bytes stay the caller's)
struct PairCross {
    std::vector<PairBlobView> blobs;
};

// the masks that take part (the rule of pair.go, lm_pair_plan.h)
static void pair_take_masks(const HostIndex &h, const std::string &who, int32_t masks, std::vector<int32_t> &sel) {
    std::string why;
    if (masks < 0 || !pair_select_masks(h.masks.data(), h.M, h.k, masks, sel, why))
        throw OptionError(who + ": " + (masks < 0 ? "masks (" + std::to_string(masks) + ") should be 0 (all masks) or a power of 4 that is >= 64" : why));
}
// the records that take part, as (key, local record), ascending by key
static std::vector<std::pair<uint64_t, int64_t>> pair_take_records(lm_index *ix, const std::string &who, const uint64_t *keys, size_t nkeys) {
    const HostIndex &h = ix->host;
    if (!keys && nkeys > 0) throw ArgError(who + ": keys is NULL but nkeys is not 0");
    const int64_t nlocal = (int64_t)h.genomes.size();
    std::vector<std::pair<uint64_t, int64_t>> chosen;
    if (!keys) {
        for (int64_t l = 0; l < nlocal; l++) chosen.emplace_back(h.genomes[(size_t)l].bg, l);
    } else {
        std::vector<uint8_t> taken((size_t)nlocal, 0);
        for (size_t s = 0; s < nkeys; s++) {
            const auto it = ix->bg2local.find(keys[s]);
            const std::string name = "key " + std::to_string(keys[s]) + " (batch " + std::to_string(keys[s] >> 17) + ", index " + std::to_string(keys[s] & 0x1ffff) + ")";
            if (it == ix->bg2local.end() && h.other_of.count(keys[s]))
                throw ArgError(who + ": " + name + " is a record of another shard (this handle is shard " + std::to_string(h.shard_rank) + " of " +
                              std::to_string(h.shard_count) + " and selects among its own records)");
            if (it == ix->bg2local.end()) throw ArgError(who + ": " + name + " is no record of this index");
            if (taken[(size_t)it->second]) throw ArgError(who + ": " + name + " is given twice");
            taken[(size_t)it->second] = 1;
            chosen.emplace_back(keys[s], (int64_t)it->second);
        }
    }
    std::sort(chosen.begin(), chosen.end());
    return chosen;
}

// k_pair_entries over the handle's own lists: count() sizes the kept seeds (n), write() places them
struct PairOwnScan {
    DBuf<int32_t> d_sel, d_slot;
    DBuf<int64_t> d_eoff, tile_off;
    DBuf<uint32_t> tile_cnt;
    PairEntArgs a;
    unsigned grid = 1;
    int64_t nraw = 0, n = 0;
    void count(lm_index *ix, const std::vector<int32_t> &sel, const std::vector<int32_t> &slot_of_local) {
        const hipStream_t st = ix->lane[0].main.st;
        const int M = ix->host.M;
        const int32_t ns = (int32_t)sel.size();
        std::vector<int64_t> md_off((size_t)2 * M + 1), out_off((size_t)2 * M + 1), eoff((size_t)ns + 1, 0);
        HIPCHK(hipMemcpyAsync(md_off.data(), ix->d_md_off.p, md_off.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(out_off.data(), ix->d_out_off.p, out_off.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int32_t s = 0; s < ns; s++) {
            const size_t md = (size_t)2 * sel[(size_t)s];
            eoff[(size_t)s + 1] = eoff[(size_t)s] + (md_off[md + 1] - md_off[md]) + (out_off[md + 1] - out_off[md]);
        }
        nraw = eoff.back();
        const int64_t ntiles = (nraw + 255) / 256;
        auto up = [&](auto &dbuf, const auto &vec) {
            dbuf.alloc_exact(std::max<size_t>(vec.size(), 1));
            if (!vec.empty()) HIPCHK(hipMemcpyAsync(dbuf.p, vec.data(), vec.size() * sizeof(vec[0]), hipMemcpyHostToDevice, st));
        };
        up(d_sel, sel);
        up(d_slot, slot_of_local);
        up(d_eoff, eoff);
        HIPCHK(hipStreamSynchronize(st)); // (the vectors end with this call)
        n = 0;
        if (nraw == 0) return;
        tile_cnt.alloc_exact((size_t)ntiles + 1, true, st);
        tile_off.alloc_exact((size_t)ntiles + 1);
        a = PairEntArgs{d_sel.p, d_eoff.p, ns, nraw, ntiles, d_slot.p, (int64_t)slot_of_local.size(), tile_cnt.p, tile_off.p, nullptr, nullptr, nullptr, 0};
        grid = (unsigned)std::min<int64_t>(ntiles, 4096);
        hipLaunchKernelGGL((k_pair_entries<true>), dim3(grid), dim3(256), 0, st, ix->view, a);
        HIPCHK(hipGetLastError());
        prim_scan_to_i64(st, ix->lane[0].main.tmp, tile_cnt.p, (size_t)ntiles, tile_off.p);
        HIPCHK(hipMemcpyAsync(&n, tile_off.p + ntiles, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    void write(lm_index *ix, uint64_t *e_kmer, uint32_t *e_slot, uint32_t *e_ms) { // [n] each
        if (n == 0) return;
        a.e_kmer = e_kmer;
        a.e_slot = e_slot;
        a.e_ms = e_ms;
        a.cap = n;
        hipLaunchKernelGGL((k_pair_entries<false>), dim3(grid), dim3(256), 0, ix->lane[0].main.st, ix->view, a);
        HIPCHK(hipGetLastError());
    }
};

// cross == nullptr: lm_index_genome_pairs.  Otherwise lm_index_genome_pairs_across: the rows with at least one own record.
static void pairs_run(lm_index *ix, const uint64_t *keys, size_t nkeys, const lm_pair_opt &opt, const PairCross *cross, PairOut &out) {
    const std::string who = cross ? "lm_index_genome_pairs_across" : "lm_index_genome_pairs";
    const hipStream_t st = ix->lane[0].main.st;
    DBuf<uint8_t> &tmp = ix->lane[0].main.tmp;
    const HostIndex &h = ix->host;
    const int K = h.k, M = h.M;
    const bool dbg = getenv("LM_DEBUG") != nullptr;
    const double t_begin = now_ms();
    // ---- refusals
    if (!cross && h.shard_count > 1)
        throw ArgError(who + ": this handle is shard " + std::to_string(h.shard_rank) + " of " + std::to_string(h.shard_count) +
                      "; a shard does not see the pairs across shards, so the pairs of an index are computed on an unsharded handle");
    if (!keys && nkeys > 0) throw ArgError(who + ": keys is NULL but nkeys is not 0");
    if (opt.min_prefix > K || opt.min_prefix < h.mask_prefix + h.anchor_prefix)
        throw OptionError(who + ": min_prefix (" + std::to_string(opt.min_prefix) + ") should be in the range of [" +
                         std::to_string(h.mask_prefix + h.anchor_prefix) + ", " + std::to_string(K) + "]");
    if (!(opt.min_mask_fraction >= 0.0))
        throw OptionError(who + ": min_mask_fraction (" + std::to_string(opt.min_mask_fraction) + ") should be >= 0");
    std::vector<int32_t> sel;
    pair_take_masks(h, who, opt.masks, sel);
    const int32_t ns = (int32_t)sel.size();
    const int64_t required = pair_required(opt.min_mask_fraction, ns);
    out.stats.total_masks = ns;
    out.stats.required = required;
    // ---- the selection: slots in ascending key order, so that ascending pairs are ascending (key1, key2)
    const int64_t nlocal = (int64_t)h.genomes.size();
    const std::vector<std::pair<uint64_t, int64_t>> chosen = pair_take_records(ix, who, keys, nkeys);
    const int64_t nown = (int64_t)chosen.size();
    std::vector<int32_t> slot_of_local((size_t)nlocal, -1);
    PairSlots slots; // (across only)
    int64_t nblob_entries = 0;
    if (!cross) {
        out.slot_key.resize((size_t)nown);
        for (int64_t s = 0; s < nown; s++) {
            slot_of_local[(size_t)chosen[(size_t)s].second] = (int32_t)s;
            out.slot_key[(size_t)s] = chosen[(size_t)s].first;
        }
    } else {
        const uint64_t fp = pair_mask_fingerprint(h.masks.data(), M);
        std::vector<uint64_t> own((size_t)nown);
        std::vector<std::vector<uint64_t>> bkeys(cross->blobs.size());
        for (int64_t s = 0; s < nown; s++) own[(size_t)s] = chosen[(size_t)s].first;
        std::string why;
        for (size_t b = 0; b < cross->blobs.size(); b++) {
            const PairBlobView &bv = cross->blobs[b];
            if (!pair_blob_fits(bv.hd, K, M, fp, opt.masks, ns, why)) throw ArgError(who + ": blob " + std::to_string(b) + ": " + why);
            bkeys[b].resize((size_t)bv.hd.records);
            if (bv.hd.records) memcpy(bkeys[b].data(), bv.keys, (size_t)bv.hd.records * 8);
            nblob_entries += bv.hd.entries;
        }
        if (!pair_slot_union(own, bkeys, slots, why)) throw ArgError(who + ": " + why);
        for (int64_t s = 0; s < nown; s++) slot_of_local[(size_t)chosen[(size_t)s].second] = (int32_t)slots.own_slot[(size_t)s];
        out.slot_key = slots.key;
        out.slot_src = slots.src;
        out.slot_idx = slots.idx;
        for (int64_t s = 0; s < (int64_t)slots.key.size(); s++)
            if (slots.src[(size_t)s] < 0) out.slot_idx[(size_t)s] = chosen[(size_t)slots.idx[(size_t)s]].second; // (own: the local record)
    }
    const int64_t nsel = (int64_t)out.slot_key.size();
    if (nsel < 2 || ns == 0 || nown == 0) { // no two records, or no own one: no pair
        out.stats.ms_total = now_ms() - t_begin;
        return;
    }
    if (nsel >= ((int64_t)1 << 31)) throw ArgError(who + ": more than 2^31 records");
    const int slot_bits = pair_bits(nsel);
    // ---- entries
    PairOwnScan own;
    own.count(ix, sel, slot_of_local);
    int64_t n = own.n + nblob_entries;
    const bool two = nblob_entries > 0; // (without blob entries the own ones are in group order as they are)
    DBuf<uint64_t> e_kmer;
    DBuf<uint32_t> e_slot, e_ms, cnt, back;
    DBuf<int64_t> offs, ceoff, d_tot;
    std::vector<int64_t> h_ceoff((size_t)ns + 1, 0), h_tot((size_t)ns, 0);
    if (n > 0) {
        DBuf<int64_t> hp;
        if (!two) {
            try {
                e_kmer.alloc_exact((size_t)n);
                e_slot.alloc_exact((size_t)n);
                e_ms.alloc_exact((size_t)n);
                cnt.alloc_exact((size_t)n + 1);
                offs.alloc_exact((size_t)n + 1);
                hp.alloc_exact((size_t)n);
            } catch (const DeviceOOM &e) {
                throw DeviceOOM(who + ": the " + std::to_string((long long)n) + " forward seeds of the selected masks and records need 36 B each (" +
                                std::to_string((n * 36) >> 20) + " MB) on the device beside the index: " + e.what() + "; select fewer masks or records");
            }
            own.write(ix, e_kmer.p, e_slot.p, e_ms.p);
            hipLaunchKernelGGL(k_pair_heads, dim3(grid_for(n)), dim3(256), 0, st, e_kmer.p, e_ms.p, n, (K - opt.min_prefix) << 1, hp.p);
            HIPCHK(hipGetLastError());
            pr_max_scan(st, tmp, hp.p, (size_t)n);
            hipLaunchKernelGGL(k_pair_counts, dim3(grid_for(n + 1)), dim3(256), 0, st, hp.p, n, cnt.p);
            HIPCHK(hipGetLastError());
        } else {
            // own entries, then every blob's: a stable sort by the top min_prefix bases and a stable sort by mask bring the
            // groups together and keep the own entries of a group ahead of its blob entries
            const auto oom = [&](const DeviceOOM &e, int per) {
                return DeviceOOM(who + ": the " + std::to_string((long long)n) + " forward seeds of the selected masks and records (" + std::to_string((long long)own.n) +
                                 " own, " + std::to_string((long long)nblob_entries) + " of the blobs) need " + std::to_string(per) + " B each (" +
                                 std::to_string((n * per) >> 20) + " MB) and the radix sort's scratch on the device beside the index: " + e.what() +
                                 "; select fewer masks or records");
            };
            DBuf<uint64_t> pk, k2, v2;
            DBuf<uint8_t> ownf;
            DBuf<int64_t> ownx;
            try {
                e_kmer.alloc_exact((size_t)n);
                pk.alloc_exact((size_t)n);
                k2.alloc_exact((size_t)n);
                v2.alloc_exact((size_t)n);
            } catch (const DeviceOOM &e) {
                throw oom(e, 32);
            }
            if (own.n > 0) { // (k2 / v2 are staging room until the sort)
                uint32_t *os = (uint32_t *)v2.p, *om = os + own.n;
                own.write(ix, e_kmer.p, os, om);
                hipLaunchKernelGGL(k_pair_pack_own, dim3(grid_for(own.n)), dim3(256), 0, st, os, om, own.n, pk.p);
                HIPCHK(hipGetLastError());
            }
            int64_t at = own.n;
            DBuf<int64_t> b_eoff;
            DBuf<uint32_t> b_slot;
            for (size_t b = 0; b < cross->blobs.size(); b++) {
                const PairBlobView &bv = cross->blobs[b];
                const int64_t nb = bv.hd.entries;
                if (nb == 0) continue;
                uint32_t *rec = (uint32_t *)k2.p + at;
                b_eoff.ensure((size_t)ns + 1);
                b_slot.ensure((size_t)bv.hd.records);
                HIPCHK(hipMemcpyAsync(e_kmer.p + at, bv.kmers, (size_t)nb * 8, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(rec, bv.recs, (size_t)nb * 4, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(b_eoff.p, bv.offsets, ((size_t)ns + 1) * 8, hipMemcpyHostToDevice, st));
                HIPCHK(hipMemcpyAsync(b_slot.p, slots.blob_slot[b].data(), (size_t)bv.hd.records * 4, hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(k_pair_pack_blob, dim3(grid_for(nb)), dim3(256), 0, st, rec, nb, b_eoff.p, ns, b_slot.p, bv.hd.records, pk.p + at);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st)); // (b_eoff / b_slot serve the next blob)
                at += nb;
            }
            prim_sort_pairs(st, tmp, e_kmer.p, k2.p, pk.p, v2.p, (size_t)n, (K - opt.min_prefix) << 1, K << 1);
            prim_sort_pairs(st, tmp, v2.p, pk.p, k2.p, e_kmer.p, (size_t)n, 32, 32 + std::max(1, pair_bits(ns)));
            HIPCHK(hipStreamSynchronize(st));
            k2.release();
            v2.release();
            try {
                e_slot.alloc_exact((size_t)n);
                e_ms.alloc_exact((size_t)n);
                ownf.alloc_exact((size_t)n + 1);
                hipLaunchKernelGGL(k_pair_unpack, dim3(grid_for(n + 1)), dim3(256), 0, st, pk.p, n, e_slot.p, e_ms.p, ownf.p);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st));
                pk.release();
                cnt.alloc_exact((size_t)n + 1);
                back.alloc_exact((size_t)n);
                offs.alloc_exact((size_t)n + 1);
                hp.alloc_exact((size_t)n);
                ownx.alloc_exact((size_t)n + 1);
            } catch (const DeviceOOM &e) {
                throw oom(e, 49);
            }
            hipLaunchKernelGGL(k_pair_heads, dim3(grid_for(n)), dim3(256), 0, st, e_kmer.p, e_ms.p, n, (K - opt.min_prefix) << 1, hp.p);
            HIPCHK(hipGetLastError());
            pr_max_scan(st, tmp, hp.p, (size_t)n);
            prim_scan_to_i64(st, tmp, ownf.p, (size_t)n, ownx.p);
            hipLaunchKernelGGL(k_pair_counts_two, dim3(grid_for(n + 1)), dim3(256), 0, st, hp.p, ownx.p, n, cnt.p, back.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st)); // (ownf / ownx end here)
        }
        prim_scan_to_i64(st, tmp, cnt.p, (size_t)n, offs.p);
        ceoff.alloc_exact((size_t)ns + 1);
        d_tot.alloc_exact((size_t)ns);
        hipLaunchKernelGGL(k_pair_mask_bounds, dim3(grid_for(n + 1)), dim3(256), 0, st, e_ms.p, n, ns, ceoff.p);
        hipLaunchKernelGGL(k_pair_mask_totals, dim3(grid_for(ns)), dim3(256), 0, st, ceoff.p, offs.p, ns, d_tot.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_ceoff.data(), ceoff.p, h_ceoff.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(h_tot.data(), d_tot.p, h_tot.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    out.stats.entries = n;
    const double t_entries = now_ms();
    out.stats.ms_entries = t_entries - t_begin;
    // ---- pieces of whole masks
    size_t fr_b = 0, tot_b = 0;
    HIPCHK(hipMemGetInfo(&fr_b, &tot_b));
    const int64_t per_tuple = 25 + 16; // (two key arrays, flag, scan; the radix sort's scratch with room to spare)
    const int64_t hard = std::max<int64_t>(1024, ((int64_t)fr_b - ((int64_t)1 << 30)) / per_tuple);
    int64_t soft = std::min<int64_t>(hard, (int64_t)1 << 26);
    if (const char *e = getenv("LM_PAIR_PIECE_TUPLES")) soft = std::min<int64_t>(hard, std::max<int64_t>(1, atoll(e)));
    std::vector<PairPiece> pieces;
    int32_t bad = 0;
    if (!pair_pieces(h_tot.data(), ns, soft, hard, slot_bits, pieces, &bad)) {
        if (bad < 0)
            throw ArgError(std::string(who) + ": two of " + std::to_string((long long)nsel) + " record slots and a length do not fit a 64-bit tuple: select at most 2^29 records");
        throw DeviceOOM(std::string(who) + ": mask " + std::to_string(sel[(size_t)bad]) + " alone gives " + std::to_string((long long)h_tot[(size_t)bad]) +
                        " candidate seed pairs; at " + std::to_string((long long)per_tuple) + " B each the tuples of one mask must fit the " +
                        std::to_string(fr_b >> 20) + " MB free beside the index: select fewer records or a longer min_prefix");
    }
    std::vector<int64_t> tfirst((size_t)ns + 1, 0);
    for (int32_t s = 0; s < ns; s++) tfirst[(size_t)s + 1] = tfirst[(size_t)s] + h_tot[(size_t)s];
    // ---- per piece: emit, sort, reduce, accumulate.  The table: tab_pair / tab_val [nt], ascending by pair.
    DBuf<uint64_t> tk, tk2, tab_pair, cat_pair, cat_pair2;
    DBuf<unsigned long long> tab_val, cat_val, cat_val2;
    DBuf<uint8_t> fr, fh, fk;
    DBuf<int64_t> orr, pos_h, pos_k;
    int64_t nt = 0;
    const int pair_bits_all = 2 * slot_bits;
    // the nr partial rows that lie at cat_*[nt ..) (the table was copied to cat_*[0 .. nt)) join the table
    auto accumulate = [&](int64_t nr, int64_t masks_left) {
        const int64_t nc = nt + nr;
        if (nc == 0) return;
        const uint64_t *sp = cat_pair.p;
        const unsigned long long *sv = cat_val.p;
        if (nt > 0 && nr > 0) {
            cat_pair2.ensure((size_t)nc);
            cat_val2.ensure((size_t)nc);
            prim_sort_pairs(st, tmp, cat_pair.p, cat_pair2.p, cat_val.p, cat_val2.p, (size_t)nc, 0, std::max(1, pair_bits_all));
            sp = cat_pair2.p;
            sv = cat_val2.p;
        }
        fh.ensure((size_t)nc + 1);
        fk.ensure((size_t)nc + 1);
        pos_h.ensure((size_t)nc + 1);
        pos_k.ensure((size_t)nc + 1);
        hipLaunchKernelGGL(k_pair_merge_flags, dim3(grid_for(nc + 1)), dim3(256), 0, st, sp, sv, nc, masks_left, required, fh.p, fk.p);
        HIPCHK(hipGetLastError());
        prim_scan_to_i64(st, tmp, fh.p, (size_t)nc, pos_h.p);
        prim_scan_to_i64(st, tmp, fk.p, (size_t)nc, pos_k.p);
        int64_t heads = 0, kept = 0;
        HIPCHK(hipMemcpyAsync(&heads, pos_h.p + nc, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&kept, pos_k.p + nc, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        out.stats.pairs_seen += heads - nt; // pairs the table did not hold before this piece
        tab_pair.ensure((size_t)std::max<int64_t>(kept, 1));
        tab_val.ensure((size_t)std::max<int64_t>(kept, 1));
        hipLaunchKernelGGL(k_pair_merge_scatter, dim3(grid_for(nc)), dim3(256), 0, st, sp, sv, nc, fk.p, pos_k.p, tab_pair.p, tab_val.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        nt = kept;
    };
    bool filtered = false;
    for (const PairPiece &P : pieces) {
        if (P.tuples == 0) continue;
        const double ta = now_ms();
        const int64_t e0 = h_ceoff[(size_t)P.s0], e1 = h_ceoff[(size_t)P.s1], tbase = tfirst[(size_t)P.s0], nall = P.tuples;
        const int key_bits = pair_key_bits(slot_bits, P.mask_bits), pair_shift = P.mask_bits + LM_PAIR_LEN_BITS;
        if (key_bits > 64 || tfirst[(size_t)P.s1] - tbase != nall || e1 <= e0) throw HipError(std::string(who) + ": a piece does not fit its plan");
        out.stats.pieces++;
        out.stats.tuples += nall;
        try {
            tk.ensure((size_t)nall);
            tk2.ensure((size_t)nall);
            fr.ensure((size_t)nall + 1);
            orr.ensure((size_t)nall + 1);
        } catch (const DeviceOOM &e) {
            throw DeviceOOM(std::string(who) + ": the " + std::to_string((long long)nall) + " tuples of masks " + std::to_string(sel[(size_t)P.s0]) + " .. " +
                            std::to_string(sel[(size_t)P.s1 - 1]) + " need 25 B each on the device beside the index: " + e.what());
        }
        const unsigned grid = (unsigned)std::min<int64_t>((nall + 255) / 256, 1 << 16);
        if (two)
            hipLaunchKernelGGL((k_pair_emit<true>), dim3(grid), dim3(256), 0, st, e_kmer.p, e_slot.p, e_ms.p, cnt.p, back.p, offs.p, e0, e1, tbase, nall,
                               (uint32_t)P.s0, K, slot_bits, P.mask_bits, tk.p);
        else
            hipLaunchKernelGGL((k_pair_emit<false>), dim3(grid), dim3(256), 0, st, e_kmer.p, e_slot.p, e_ms.p, cnt.p, (const uint32_t *)nullptr, offs.p, e0, e1,
                               tbase, nall, (uint32_t)P.s0, K, slot_bits, P.mask_bits, tk.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        const double tb = now_ms();
        out.stats.ms_emit += tb - ta;
        prim_sort_keys(st, tmp, tk.p, tk2.p, (size_t)nall, 0, key_bits);
        hipLaunchKernelGGL(k_pair_flags, dim3(grid_for(nall + 1)), dim3(256), 0, st, tk2.p, nall, pair_shift, fr.p);
        HIPCHK(hipGetLastError());
        prim_scan_to_i64(st, tmp, fr.p, (size_t)nall, orr.p);
        int64_t nr = 0;
        HIPCHK(hipMemcpyAsync(&nr, orr.p + nall, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        try {
            cat_pair.ensure((size_t)std::max<int64_t>(nt + nr, 1));
            cat_val.ensure((size_t)std::max<int64_t>(nt + nr, 1));
        } catch (const DeviceOOM &e) {
            throw DeviceOOM(std::string(who) + ": the pair table of " + std::to_string((long long)(nt + nr)) + " rows needs 32 B per row and the radix sort's scratch "
                            "on the device beside the index: " + e.what() + "; raise min_mask_fraction or min_prefix");
        }
        if (nt > 0) {
            HIPCHK(hipMemcpyAsync(cat_pair.p, tab_pair.p, (size_t)nt * 8, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(cat_val.p, tab_val.p, (size_t)nt * 8, hipMemcpyDeviceToDevice, st));
        }
        if (nr > 0) {
            HIPCHK(hipMemsetAsync(cat_val.p + nt, 0, (size_t)nr * 8, st));
            hipLaunchKernelGGL(k_pair_reduce, dim3(grid_for((nall + PR_RUN - 1) / PR_RUN)), dim3(256), 0, st, tk2.p, nall, pair_shift, fr.p, orr.p,
                               cat_pair.p + nt, cat_val.p + nt);
            HIPCHK(hipGetLastError());
        }
        accumulate(nr, (int64_t)ns - P.s1);
        filtered = P.s1 == ns;
        out.stats.ms_reduce += now_ms() - tb;
        if (dbg)
            fprintf(stderr, "[lm] pairs: masks %d .. %d, %lld tuples, %lld partial rows, table %lld\n", (int)sel[(size_t)P.s0], (int)sel[(size_t)P.s1 - 1],
                    (long long)nall, (long long)nr, (long long)nt);
    }
    if (!filtered && nt > 0) { // (the last masks had no tuples: the filter by `required` is the prune with nothing left)
        cat_pair.ensure((size_t)nt);
        cat_val.ensure((size_t)nt);
        HIPCHK(hipMemcpyAsync(cat_pair.p, tab_pair.p, (size_t)nt * 8, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(cat_val.p, tab_val.p, (size_t)nt * 8, hipMemcpyDeviceToDevice, st));
        accumulate(0, 0);
    }
    // ---- finish: the rule's order, rows to the host
    out.stats.rows = nt;
    if (nt > 0) {
        cat_pair.ensure((size_t)nt);
        cat_pair2.ensure((size_t)nt);
        cat_val.ensure((size_t)nt);
        cat_val2.ensure((size_t)nt);
        uint64_t *okey = cat_pair.p, *okey2 = cat_pair2.p;
        hipLaunchKernelGGL(k_pair_order_keys, dim3(grid_for(nt)), dim3(256), 0, st, tab_val.p, nt, okey);
        HIPCHK(hipGetLastError());
        prim_sort_pairs(st, tmp, okey, okey2, tab_pair.p, (uint64_t *)cat_val2.p, (size_t)nt, 0, 64);
        std::vector<uint64_t> hk((size_t)nt), hp((size_t)nt);
        HIPCHK(hipMemcpyAsync(hk.data(), okey2, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(hp.data(), cat_val2.p, (size_t)nt * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        out.rows.resize((size_t)nt);
        const uint64_t sm = ((uint64_t)1 << slot_bits) - 1;
        for (int64_t i = 0; i < nt; i++) {
            const uint64_t val = ~hk[(size_t)i];
            out.rows[(size_t)i] = PairRow{((hp[(size_t)i] >> slot_bits) << 32) | (hp[(size_t)i] & sm), (uint32_t)(val >> 32), (uint32_t)val};
        }
    }
    tmp.release();
    out.stats.ms_total = now_ms() - t_begin;
}

} // namespace lm

struct lm_pairs {
    std::vector<lm_pair_row> rows;
    lm_pair_stats stats;
    std::deque<std::string> owned; // names the result owns: blob records (lm_index_genome_pairs_across), every name of a merge
};

extern "C" void lm_pair_opt_default(lm_pair_opt *o) {
    if (!o) return;
    o->min_prefix = 21;
    o->masks = 1024;
    o->min_mask_fraction = 0.25;
}

// lm::guarded's text, behind the call's name, for a host that ran out of memory: every call of this file
static const char *const PAIRS_NOMEM = ": the host could not hold the selection or the rows";

// lm_index_genome_pairs (cross == nullptr) and lm_index_genome_pairs_across
static lm_status pairs_call(lm_index *ix, const char *who, const uint64_t *keys, size_t nkeys, const lm_pair_opt *opt_in, const lm::PairCross *cross,
                            lm_pairs **out) {
    using namespace lm;
    lm_pair_opt opt;
    lm_pair_opt_default(&opt);
    if (opt_in) opt = *opt_in;
    std::unique_ptr<lm_pairs> res(new lm_pairs());
    memset(&res->stats, 0, sizeof res->stats);
    const lm_status rc = guarded(ix, who, PAIRS_NOMEM, [&]() {
        PairOut po;
        memset(&po.stats, 0, sizeof po.stats);
        pairs_run(ix, keys, nkeys, opt, cross, po);
        // names: one lookup per record that is in a row; a blob record's id is copied into the result
        std::vector<uint8_t> used(po.slot_key.size(), 0);
        for (const PairRow &r : po.rows) used[(size_t)(r.pair >> 32)] = used[(size_t)(r.pair & 0xffffffffu)] = 1;
        std::vector<uint64_t> own_keys;
        std::vector<int64_t> name_of(po.slot_key.size(), -1);
        std::vector<const char *> name;
        std::vector<std::vector<int64_t>> id_off(cross ? cross->blobs.size() : 0); // per blob with a used record: where its ids start
        for (size_t s = 0; s < used.size(); s++) {
            if (!used[s]) continue;
            if (po.slot_src.empty() || po.slot_src[s] < 0) {
                name_of[s] = (int64_t)own_keys.size();
                own_keys.push_back(po.slot_key[s]);
            }
        }
        genome_ids_of_keys(ix, own_keys, name);
        for (size_t s = 0; s < used.size(); s++) {
            if (!used[s] || name_of[s] >= 0) continue;
            const size_t b = (size_t)po.slot_src[s];
            const PairBlobView &bv = cross->blobs[b];
            if (id_off[b].empty()) {
                id_off[b].assign((size_t)bv.hd.records + 1, 0);
                for (int64_t r = 0; r < bv.hd.records; r++) id_off[b][(size_t)r + 1] = id_off[b][(size_t)r] + bv.idlen(r);
            }
            const int64_t r = po.slot_idx[s];
            res->owned.emplace_back((const char *)bv.ids + id_off[b][(size_t)r], (size_t)bv.idlen(r));
            name_of[s] = (int64_t)name.size();
            name.push_back(res->owned.back().c_str());
        }
        res->rows.resize(po.rows.size());
        for (size_t i = 0; i < po.rows.size(); i++) {
            const size_t s1 = (size_t)(po.rows[i].pair >> 32), s2 = (size_t)(po.rows[i].pair & 0xffffffffu);
            lm_pair_row &o = res->rows[i];
            memset(&o, 0, sizeof o);
            o.key1 = po.slot_key[s1];
            o.key2 = po.slot_key[s2];
            o.genome1 = name[(size_t)name_of[s1]];
            o.genome2 = name[(size_t)name_of[s2]];
            o.n_masks = po.rows[i].n_masks;
            o.sum_prefix = po.rows[i].sum_prefix;
        }
        res->stats = po.stats;
    });
    if (rc != LM_OK) return rc;
    *out = res.release();
    return LM_OK;
}

extern "C" lm_status lm_index_genome_pairs(lm_index *ix, const uint64_t *keys, size_t nkeys, const lm_pair_opt *opt_in, lm_pairs **out) {
    if (!ix || !out) return LM_ERR_ARG;
    *out = nullptr;
    return pairs_call(ix, "lm_index_genome_pairs", keys, nkeys, opt_in, nullptr, out);
}

extern "C" lm_status lm_index_genome_pairs_across(lm_index *ix, const uint64_t *keys, size_t nkeys, const void *const *blobs, const size_t *blob_bytes,
                                                  size_t nblobs, const lm_pair_opt *opt_in, lm_pairs **out) {
    using namespace lm;
    if (!ix || !out) return LM_ERR_ARG;
    *out = nullptr;
    const char *who = "lm_index_genome_pairs_across";
    PairCross cross;
    if (nblobs > 0 && (!blobs || !blob_bytes)) {
        std::lock_guard<std::mutex> lock(ix->mu);
        ix->err = std::string(who) + ": blobs or blob_bytes is NULL but nblobs is not 0";
        return LM_ERR_ARG;
    }
    cross.blobs.resize(nblobs);
    for (size_t b = 0; b < nblobs; b++) {
        std::string why;
        if (!pair_blob_parse(blobs[b], blob_bytes[b], cross.blobs[b], why)) {
            std::lock_guard<std::mutex> lock(ix->mu);
            ix->err = std::string(who) + ": blob " + std::to_string(b) + ": " + why;
            return LM_ERR_ARG;
        }
    }
    return pairs_call(ix, who, keys, nkeys, opt_in, &cross, out);
}

// the forward seeds of the taken masks of the selected records, for the other shards (layout: lm_pair_cross_plan.h)
extern "C" lm_status lm_index_pair_seeds(lm_index *ix, const uint64_t *keys, size_t nkeys, const lm_pair_opt *opt_in, void **blob, size_t *bytes) {
    using namespace lm;
    if (!ix || !blob || !bytes) return LM_ERR_ARG;
    *blob = nullptr;
    *bytes = 0;
    const std::string who = "lm_index_pair_seeds";
    lm_pair_opt opt;
    lm_pair_opt_default(&opt);
    if (opt_in) opt = *opt_in;
    return guarded(ix, who.c_str(), PAIRS_NOMEM, [&]() {
        const hipStream_t st = ix->lane[0].main.st;
        const HostIndex &h = ix->host;
        std::vector<int32_t> sel;
        pair_take_masks(h, who, opt.masks, sel);
        const int32_t ns = (int32_t)sel.size();
        const std::vector<std::pair<uint64_t, int64_t>> chosen = pair_take_records(ix, who, keys, nkeys);
        const int64_t nrec = (int64_t)chosen.size();
        if (nrec > LM_PAIR_MAX_SLOTS) throw ArgError(who + ": more than 2^29 records");
        // slots in ascending key order: a seed's slot is its record's index in the blob
        std::vector<int32_t> slot_of_local(h.genomes.size(), -1);
        std::vector<uint64_t> rkeys((size_t)nrec);
        for (int64_t s = 0; s < nrec; s++) {
            slot_of_local[(size_t)chosen[(size_t)s].second] = (int32_t)s;
            rkeys[(size_t)s] = chosen[(size_t)s].first;
        }
        std::vector<uint64_t> kmers;
        std::vector<uint32_t> recs;
        std::vector<int64_t> offsets((size_t)ns + 1, 0);
        if (nrec > 0 && ns > 0) {
            PairOwnScan own;
            own.count(ix, sel, slot_of_local);
            const int64_t n = own.n;
            if (n > 0) {
                DBuf<uint64_t> e_kmer;
                DBuf<uint32_t> e_slot, e_ms;
                DBuf<int64_t> ceoff;
                try {
                    e_kmer.alloc_exact((size_t)n);
                    e_slot.alloc_exact((size_t)n);
                    e_ms.alloc_exact((size_t)n);
                } catch (const DeviceOOM &e) {
                    throw DeviceOOM(who + ": the " + std::to_string((long long)n) + " forward seeds of the selected masks and records need 16 B each (" +
                                    std::to_string((n * 16) >> 20) + " MB) on the device beside the index: " + e.what() + "; select fewer masks or records");
                }
                own.write(ix, e_kmer.p, e_slot.p, e_ms.p);
                ceoff.alloc_exact((size_t)ns + 1);
                hipLaunchKernelGGL(k_pair_mask_bounds, dim3(grid_for(n + 1)), dim3(256), 0, st, e_ms.p, n, ns, ceoff.p);
                HIPCHK(hipGetLastError());
                kmers.resize((size_t)n);
                recs.resize((size_t)n);
                HIPCHK(hipMemcpyAsync(kmers.data(), e_kmer.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(recs.data(), e_slot.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
                HIPCHK(hipMemcpyAsync(offsets.data(), ceoff.p, offsets.size() * 8, hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
            }
            ix->lane[0].main.tmp.release();
        }
        std::vector<const char *> idp;
        genome_ids_of_keys(ix, rkeys, idp);
        std::vector<std::string> ids((size_t)nrec);
        PairBlobHead hd;
        hd.k = h.k;
        hd.M = h.M;
        hd.masks = opt.masks;
        hd.total_masks = ns;
        hd.fingerprint = pair_mask_fingerprint(h.masks.data(), h.M);
        hd.records = nrec;
        hd.entries = (int64_t)kmers.size();
        for (int64_t s = 0; s < nrec; s++) {
            ids[(size_t)s] = idp[(size_t)s] ? idp[(size_t)s] : "";
            hd.id_bytes += (int64_t)ids[(size_t)s].size();
        }
        const size_t nb = pair_blob_size(ns, nrec, hd.entries, hd.id_bytes);
        uint8_t *p = (uint8_t *)malloc(nb);
        if (!p) throw std::bad_alloc();
        std::string why;
        if (!pair_blob_write(hd, rkeys.data(), ids, offsets.data(), kmers.data(), recs.data(), p, why)) {
            free(p);
            throw ArgError(who + ": " + why);
        }
        *blob = p;
        *bytes = nb;
    });
}

// rows that came over the wire as a result of their own: the rows and their names are copied
extern "C" lm_status lm_pairs_from_rows(const lm_pair_row *rows, size_t n, const lm_pair_stats *stats, lm_pairs **out) {
    if (!out || (!rows && n > 0)) return LM_ERR_ARG;
    *out = nullptr;
    try {
        std::unique_ptr<lm_pairs> res(new lm_pairs());
        memset(&res->stats, 0, sizeof res->stats);
        if (stats) res->stats = *stats;
        res->stats.rows = (int64_t)n;
        res->rows.assign(rows, rows + n);
        std::unordered_map<uint64_t, const char *> seen;
        for (lm_pair_row &r : res->rows)
            for (int side = 0; side < 2; side++) {
                const uint64_t key = side ? r.key2 : r.key1;
                const char *&src = side ? r.genome2 : r.genome1;
                auto it = seen.find(key);
                if (it == seen.end()) {
                    res->owned.emplace_back(src ? src : "");
                    it = seen.emplace(key, res->owned.back().c_str()).first;
                }
                src = it->second;
            }
        *out = res.release();
    } catch (const std::bad_alloc &) {
        g_open_error = "lm_pairs_from_rows: the host could not hold the rows";
        return LM_ERR_NOMEM;
    }
    return LM_OK;
}

// the ranks' rows as one result in the rule's order (lm_pair_cross_plan.h); every name is copied
extern "C" lm_status lm_pairs_merge(const lm_pairs *const *parts, size_t n, lm_pairs **out) {
    using namespace lm;
    if (!out) return LM_ERR_ARG;
    *out = nullptr;
    if (n > 0 && !parts) {
        g_open_error = "lm_pairs_merge: parts is NULL but n is not 0";
        return LM_ERR_ARG;
    }
    try {
        std::vector<const lm_pair_row *> rp(n);
        std::vector<size_t> rn(n);
        std::unique_ptr<lm_pairs> res(new lm_pairs());
        memset(&res->stats, 0, sizeof res->stats);
        for (size_t p = 0; p < n; p++) {
            if (!parts[p]) {
                g_open_error = "lm_pairs_merge: part " + std::to_string(p) + " is NULL";
                return LM_ERR_ARG;
            }
            rp[p] = parts[p]->rows.data();
            rn[p] = parts[p]->rows.size();
            const lm_pair_stats &s = parts[p]->stats;
            lm_pair_stats &o = res->stats;
            o.total_masks = std::max(o.total_masks, s.total_masks);
            o.required = std::max(o.required, s.required);
            o.entries += s.entries;
            o.tuples += s.tuples;
            o.pieces += s.pieces;
            o.pairs_seen += s.pairs_seen;
            o.ms_entries += s.ms_entries;
            o.ms_emit += s.ms_emit;
            o.ms_reduce += s.ms_reduce;
            o.ms_total += s.ms_total;
        }
        std::vector<std::pair<uint32_t, size_t>> order;
        std::string why;
        if (!pair_merge_plan(rp.data(), rn.data(), n, order, why)) {
            g_open_error = "lm_pairs_merge: " + why;
            return LM_ERR_ARG;
        }
        res->rows.resize(order.size());
        std::unordered_map<uint64_t, const char *> seen;
        for (size_t i = 0; i < order.size(); i++) {
            lm_pair_row &r = res->rows[i];
            r = rp[order[i].first][order[i].second];
            for (int side = 0; side < 2; side++) {
                const uint64_t key = side ? r.key2 : r.key1;
                const char *&src = side ? r.genome2 : r.genome1;
                auto it = seen.find(key);
                if (it == seen.end()) {
                    res->owned.emplace_back(src ? src : "");
                    it = seen.emplace(key, res->owned.back().c_str()).first;
                }
                src = it->second;
            }
        }
        res->stats.rows = (int64_t)order.size();
        *out = res.release();
    } catch (const std::bad_alloc &) {
        g_open_error = "lm_pairs_merge: the host could not hold the rows";
        return LM_ERR_NOMEM;
    }
    return LM_OK;
}

extern "C" size_t lm_pairs_rows(const lm_pairs *p, const lm_pair_row **rows) {
    if (!p) return 0;
    if (rows) *rows = p->rows.data();
    return p->rows.size();
}
extern "C" void lm_pairs_get_stats(const lm_pairs *p, lm_pair_stats *s) {
    if (p && s) *s = p->stats;
}
extern "C" void lm_pairs_free(lm_pairs *p) { delete p; }

// pair.go:730
extern "C" int lm_format_pair_row(const lm_pair_row *r, int min_prefix, int total_masks, char *buf, size_t cap) {
    if (!r) return 0;
    return lm::pair_format_row(r->genome1, r->genome2, min_prefix, r->n_masks, r->sum_prefix, total_masks, buf, cap);
}
// pair.go:721
extern "C" const char *lm_pair_header(void) { return lm::pair_header(); }
