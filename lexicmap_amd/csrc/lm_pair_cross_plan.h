// lm_pair_cross_plan.h — the host's part of the pairs across shards (lm_index_pair_seeds, lm_index_genome_pairs_across,
// lm_pairs_merge in lm_pairs.hip): the seed blob a rank exports - its writer, its parser and validator -
// the slots of the union of own and blob records, and the merge of the ranks' rows.  Host-only and free of HIP, so that
// tests/pair_cross_host.cpp can run it under the sanitizers; nothing here trusts a byte of a blob before it is checked.
//
// The blob, little-endian throughout, no alignment needed (every field is copied out):
//   uint64 magic; int32 k, M = masks of the index, masks = the option the selection was made with, total_masks = masks taken;
//   uint64 fingerprint of the M mask values; int64 records, entries, id_bytes;                                      (56 B)
//   uint64 keys[records], ascending; uint16 id_len[records]; char ids[id_bytes], back to back, no terminators;
//   int64 offsets[total_masks + 1]: the first entry of every taken mask, offsets[total_masks] = entries;
//   uint64 kmers[entries]; uint32 record[entries]: index into keys.  Entries in list order per mask: packed list, then outliers.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace lm {

#define LM_PAIR_BLOB_MAGIC 0x3144455352504d4cull /* "LMPRSED1" */
#define LM_PAIR_BLOB_HEAD 56
#define LM_PAIR_MAX_SLOTS ((int64_t)1 << 29)

// FNV-1a over the mask count and the mask values: two indexes pair their seeds only when they were cut by the same masks
static inline uint64_t pair_mask_fingerprint(const uint64_t *masks, int64_t M) {
    uint64_t h = 0xcbf29ce484222325ull;
    auto eat = [&h](uint64_t v) {
        for (int b = 0; b < 8; b++) {
            h ^= (v >> (8 * b)) & 0xff;
            h *= 0x100000001b3ull;
        }
    };
    eat((uint64_t)M);
    for (int64_t i = 0; i < M; i++) eat(masks[i]);
    return h;
}

template <typename T> static inline T pair_blob_get(const uint8_t *p, int64_t i = 0) {
    T v;
    memcpy(&v, p + (size_t)i * sizeof(T), sizeof(T));
    return v;
}

struct PairBlobHead {
    int32_t k = 0, M = 0, masks = 0, total_masks = 0;
    uint64_t fingerprint = 0;
    int64_t records = 0, entries = 0, id_bytes = 0;
};
// a parsed blob: the sections still lie in the caller's bytes (unaligned: read them with pair_blob_get or memcpy)
struct PairBlobView {
    PairBlobHead hd;
    const uint8_t *keys = nullptr, *id_len = nullptr, *ids = nullptr, *offsets = nullptr, *kmers = nullptr, *recs = nullptr;
    uint64_t key(int64_t r) const { return pair_blob_get<uint64_t>(keys, r); }
    uint16_t idlen(int64_t r) const { return pair_blob_get<uint16_t>(id_len, r); }
    int64_t offset(int64_t s) const { return pair_blob_get<int64_t>(offsets, s); }
    uint64_t kmer(int64_t e) const { return pair_blob_get<uint64_t>(kmers, e); }
    uint32_t rec(int64_t e) const { return pair_blob_get<uint32_t>(recs, e); }
};

static inline size_t pair_blob_size(int32_t total_masks, int64_t records, int64_t entries, int64_t id_bytes) {
    return (size_t)LM_PAIR_BLOB_HEAD + (size_t)records * 10 + (size_t)id_bytes + ((size_t)total_masks + 1) * 8 + (size_t)entries * 12;
}

// Writes the blob into dst[pair_blob_size(..)].  ids[r]: the genome id of keys[r], at most 65535 bytes (false + text otherwise);
// offsets: [total_masks + 1]; kmers / recs: [entries].
static inline bool pair_blob_write(const PairBlobHead &hd, const uint64_t *keys, const std::vector<std::string> &ids, const int64_t *offsets,
                                   const uint64_t *kmers, const uint32_t *recs, uint8_t *dst, std::string &err) {
    if ((int64_t)ids.size() != hd.records) {
        err = "the ids do not match the records";
        return false;
    }
    int64_t idb = 0;
    for (const std::string &s : ids) {
        if (s.size() > 65535) {
            err = "a genome id of " + std::to_string(s.size()) + " bytes does not fit the blob's 16-bit length";
            return false;
        }
        idb += (int64_t)s.size();
    }
    if (idb != hd.id_bytes) {
        err = "the ids do not add up to id_bytes";
        return false;
    }
    uint8_t *p = dst;
    auto put = [&p](const void *src, size_t n) {
        if (n) memcpy(p, src, n);
        p += n;
    };
    const uint64_t magic = LM_PAIR_BLOB_MAGIC;
    put(&magic, 8);
    put(&hd.k, 4);
    put(&hd.M, 4);
    put(&hd.masks, 4);
    put(&hd.total_masks, 4);
    put(&hd.fingerprint, 8);
    put(&hd.records, 8);
    put(&hd.entries, 8);
    put(&hd.id_bytes, 8);
    put(keys, (size_t)hd.records * 8);
    for (const std::string &s : ids) {
        const uint16_t l = (uint16_t)s.size();
        put(&l, 2);
    }
    for (const std::string &s : ids) put(s.data(), s.size());
    put(offsets, ((size_t)hd.total_masks + 1) * 8);
    put(kmers, (size_t)hd.entries * 8);
    put(recs, (size_t)hd.entries * 4);
    return (size_t)(p - dst) == pair_blob_size(hd.total_masks, hd.records, hd.entries, hd.id_bytes);
}

// Parses and checks a blob on its own: magic, counts, length, keys ascending, id lengths, offsets monotone from 0 to
// `entries`, every record index in range.  false + what is wrong; `v` is then not to be used.
static inline bool pair_blob_parse(const void *blob, size_t bytes, PairBlobView &v, std::string &err) {
    const uint8_t *b = (const uint8_t *)blob;
    if (!b || bytes < LM_PAIR_BLOB_HEAD) {
        err = "its " + std::to_string(bytes) + " bytes are shorter than the header of " + std::to_string(LM_PAIR_BLOB_HEAD);
        return false;
    }
    if (pair_blob_get<uint64_t>(b) != LM_PAIR_BLOB_MAGIC) {
        err = "it is no blob of lm_index_pair_seeds (magic)";
        return false;
    }
    PairBlobHead &h = v.hd;
    h.k = pair_blob_get<int32_t>(b + 8);
    h.M = pair_blob_get<int32_t>(b + 12);
    h.masks = pair_blob_get<int32_t>(b + 16);
    h.total_masks = pair_blob_get<int32_t>(b + 20);
    h.fingerprint = pair_blob_get<uint64_t>(b + 24);
    h.records = pair_blob_get<int64_t>(b + 32);
    h.entries = pair_blob_get<int64_t>(b + 40);
    h.id_bytes = pair_blob_get<int64_t>(b + 48);
    if (h.k < 1 || h.k > 32 || h.M < 0 || h.masks < 0 || h.total_masks < 0 || h.total_masks > h.M) {
        err = "its header is broken (k " + std::to_string(h.k) + ", masks " + std::to_string(h.M) + ", selection " + std::to_string(h.masks) +
              ", taken " + std::to_string(h.total_masks) + ")";
        return false;
    }
    const size_t room = bytes - LM_PAIR_BLOB_HEAD;
    if (h.records < 0 || h.entries < 0 || h.id_bytes < 0 || (uint64_t)h.records > room / 10 || (uint64_t)h.entries > room / 12 ||
        (uint64_t)h.id_bytes > room || h.records > (int64_t)0xffffffffll) {
        err = "its counts do not fit its length (records " + std::to_string((long long)h.records) + ", entries " + std::to_string((long long)h.entries) +
              ", id bytes " + std::to_string((long long)h.id_bytes) + ", " + std::to_string(bytes) + " bytes)";
        return false;
    }
    const size_t want = pair_blob_size(h.total_masks, h.records, h.entries, h.id_bytes);
    if (want != bytes) {
        err = "its length is " + std::to_string(bytes) + " bytes, its header asks for " + std::to_string(want);
        return false;
    }
    v.keys = b + LM_PAIR_BLOB_HEAD;
    v.id_len = v.keys + (size_t)h.records * 8;
    v.ids = v.id_len + (size_t)h.records * 2;
    v.offsets = v.ids + (size_t)h.id_bytes;
    v.kmers = v.offsets + ((size_t)h.total_masks + 1) * 8;
    v.recs = v.kmers + (size_t)h.entries * 8;
    int64_t idb = 0;
    for (int64_t r = 0; r < h.records; r++) {
        if (r > 0 && v.key(r) <= v.key(r - 1)) {
            err = "its record keys are not ascending (record " + std::to_string((long long)r) + ")";
            return false;
        }
        idb += v.idlen(r);
    }
    if (idb != h.id_bytes) {
        err = "its id lengths add up to " + std::to_string((long long)idb) + ", its header says " + std::to_string((long long)h.id_bytes);
        return false;
    }
    if (v.offset(0) != 0 || v.offset(h.total_masks) != h.entries) {
        err = "its mask offsets do not run from 0 to its " + std::to_string((long long)h.entries) + " entries";
        return false;
    }
    for (int32_t s = 0; s < h.total_masks; s++)
        if (v.offset(s + 1) < v.offset(s)) {
            err = "its mask offsets are not monotone (mask " + std::to_string(s) + " of the selection)";
            return false;
        }
    for (int64_t e = 0; e < h.entries; e++)
        if ((int64_t)v.rec(e) >= h.records) {
            err = "entry " + std::to_string((long long)e) + " names record " + std::to_string(v.rec(e)) + " of " + std::to_string((long long)h.records);
            return false;
        }
    return true;
}

// a parsed blob against the handle and the call: false + what differs
static inline bool pair_blob_fits(const PairBlobHead &h, int k, int M, uint64_t fingerprint, int32_t masks, int32_t total_masks, std::string &err) {
    if (h.k != k) err = "it is of an index with k = " + std::to_string(h.k) + ", this one has k = " + std::to_string(k);
    else if (h.M != M) err = "it is of an index with " + std::to_string(h.M) + " masks, this one has " + std::to_string(M);
    else if (h.fingerprint != fingerprint) err = "it is of an index with other mask values";
    else if (h.masks != masks || h.total_masks != total_masks)
        err = "it was exported with masks = " + std::to_string(h.masks) + " (" + std::to_string(h.total_masks) + " masks taken), this call has masks = " +
              std::to_string(masks) + " (" + std::to_string(total_masks) + " taken)";
    else return true;
    return false;
}

// ---- slots.  The union of the own keys and every blob's keys (each ascending), numbered in ascending key order, so that
// ascending pairs of slots are ascending (key1, key2) over the global keys.  src[slot]: -1 = an own record, else the blob;
// idx[slot]: its number among the own keys / in that blob.  false + text: a key that is own and in a blob, or in two blobs
// (a blob given twice), or more than 2^29 records.
struct PairSlots {
    std::vector<uint64_t> key;
    std::vector<int32_t> src;
    std::vector<int64_t> idx;
    std::vector<uint32_t> own_slot;               // [own keys]
    std::vector<std::vector<uint32_t>> blob_slot; // [blob][its records]
};
static inline bool pair_slot_union(const std::vector<uint64_t> &own, const std::vector<std::vector<uint64_t>> &blobs, PairSlots &out, std::string &err) {
    size_t total = own.size();
    for (const auto &b : blobs) total += b.size();
    if ((int64_t)total > LM_PAIR_MAX_SLOTS) {
        err = "the own records and the blobs' are " + std::to_string(total) + " records together, more than 2^29";
        return false;
    }
    out.key.assign(total, 0);
    out.src.assign(total, -1);
    out.idx.assign(total, 0);
    out.own_slot.assign(own.size(), 0);
    out.blob_slot.assign(blobs.size(), {});
    for (size_t b = 0; b < blobs.size(); b++) out.blob_slot[b].assign(blobs[b].size(), 0);
    // a k-way merge by repeated minimum over the cursors: blobs are few (one per lower rank)
    std::vector<size_t> at(blobs.size() + 1, 0);
    for (size_t s = 0; s < total; s++) {
        int best = -2;
        uint64_t bk = 0;
        for (size_t c = 0; c <= blobs.size(); c++) {
            const std::vector<uint64_t> &src = c == 0 ? own : blobs[c - 1];
            if (at[c] >= src.size()) continue;
            const uint64_t k = src[at[c]];
            if (best == -2 || k < bk) {
                best = (int)c - 1;
                bk = k;
            } else if (k == bk) {
                err = "record key " + std::to_string((unsigned long long)k) + (best < 0 ? " is also an own record of the handle" : " also occurs in blob " + std::to_string(best)) +
                      " (blob " + std::to_string((int)c - 1) + ")";
                return false;
            }
        }
        const size_t c = (size_t)(best + 1);
        if (s > 0 && bk <= out.key[s - 1]) {
            err = "record keys are not ascending";
            return false;
        }
        out.key[s] = bk;
        out.src[s] = best;
        out.idx[s] = (int64_t)at[c];
        if (best < 0) out.own_slot[at[c]] = (uint32_t)s;
        else out.blob_slot[(size_t)best][at[c]] = (uint32_t)s;
        at[c]++;
    }
    return true;
}

// ---- merge.  Row: anything with key1, key2, n_masks, sum_prefix.  The rule's order (pair.go:995-1004).
template <typename Row> static inline bool pair_cross_row_less(const Row &a, const Row &b) {
    if (a.n_masks != b.n_masks) return a.n_masks > b.n_masks;
    if (a.sum_prefix != b.sum_prefix) return a.sum_prefix > b.sum_prefix;
    if (a.key1 != b.key1) return a.key1 < b.key1;
    return a.key2 < b.key2;
}
// parts[p][0 .. n[p]): each in the rule's order.  order: (part, row) of every output row.  false + text: a part out of order,
// or a pair that occurs twice (in two parts, or twice in one).
template <typename Row>
static inline bool pair_merge_plan(const Row *const *parts, const size_t *n, size_t np, std::vector<std::pair<uint32_t, size_t>> &order, std::string &err) {
    order.clear();
    size_t total = 0;
    for (size_t p = 0; p < np; p++) {
        if (n[p] > 0 && !parts[p]) {
            err = "part " + std::to_string(p) + " has rows but no row array";
            return false;
        }
        for (size_t i = 1; i < n[p]; i++)
            if (!pair_cross_row_less(parts[p][i - 1], parts[p][i])) {
                err = "part " + std::to_string(p) + " is not in the rule's order at row " + std::to_string(i) + ", or holds a pair twice";
                return false;
            }
        total += n[p];
    }
    order.reserve(total);
    // a binary heap of the parts' cursors
    std::vector<std::pair<uint32_t, size_t>> heap;
    auto after = [&](const std::pair<uint32_t, size_t> &a, const std::pair<uint32_t, size_t> &b) { // a comes after b
        const Row &x = parts[a.first][a.second], &y = parts[b.first][b.second];
        if (pair_cross_row_less(y, x)) return true;
        if (pair_cross_row_less(x, y)) return false;
        return a.first > b.first;
    };
    for (size_t p = 0; p < np; p++)
        if (n[p] > 0) heap.emplace_back((uint32_t)p, (size_t)0);
    std::make_heap(heap.begin(), heap.end(), after);
    while (!heap.empty()) {
        std::pop_heap(heap.begin(), heap.end(), after);
        std::pair<uint32_t, size_t> c = heap.back();
        heap.pop_back();
        order.push_back(c);
        if (++c.second < n[c.first]) {
            heap.push_back(c);
            std::push_heap(heap.begin(), heap.end(), after);
        }
    }
    // a pair in two parts need not carry the same sums, so neighbours in the output do not show it: sort the pairs
    std::vector<std::pair<uint64_t, uint64_t>> pairs;
    pairs.reserve(total);
    for (size_t p = 0; p < np; p++)
        for (size_t i = 0; i < n[p]; i++) pairs.emplace_back(parts[p][i].key1, parts[p][i].key2);
    std::sort(pairs.begin(), pairs.end());
    for (size_t i = 1; i < pairs.size(); i++)
        if (pairs[i] == pairs[i - 1]) {
            err = "the pair of records " + std::to_string((unsigned long long)pairs[i].first) + " and " + std::to_string((unsigned long long)pairs[i].second) +
                  " occurs twice: every pair belongs to one part (rank r takes the blobs of the ranks s < r only)";
            return false;
        }
    return true;
}

} // namespace lm
