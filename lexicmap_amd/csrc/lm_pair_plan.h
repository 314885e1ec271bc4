// lm_pair_plan.h — the host's part of lm_index_genome_pairs (lm_pairs.hip): which masks take part, how many masks a pair
// must match in, how the selected masks are cut into pieces and how wide a piece's tuple key is, how the partial rows of the
// pieces add up and when a pair may be dropped early, the order of the rows and their text.  Host-only and free of HIP, so
// that tests/pair_plan_host.cpp can hold it to the Python model (tests/pair_model.py); the kernels are held to these loops.
// Reference: `lexicmap genome pair`, lexicmap/cmd/pair.go.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <unordered_set>
#include <vector>

namespace lm {

#define LM_PAIR_LEN_BITS 6 /* LCP <= 32 */

// bits b with 2^b >= n (n >= 1): every value in [0, n) fits b bits; 0 for n == 1
static inline int pair_bits(int64_t n) {
    int b = 0;
    while (b < 63 && ((int64_t)1 << b) < n) b++;
    return b;
}

// ---- mask selection (pair.go:162-184).  nmasks == 0: every mask.  Otherwise nmasks is a power of 4, >= 64 and <= M; with
// q = log4(nmasks) the FIRST mask (index order) of every distinct q-base prefix mask >> 2 (k - q) is taken.  false + text
// for a refused nmasks.  `sel`: the selected mask numbers ascending; its size is the rule's `total`.
static inline bool pair_select_masks(const uint64_t *masks, int M, int k, int64_t nmasks, std::vector<int32_t> &sel, std::string &err) {
    sel.clear();
    if (nmasks == 0) {
        for (int m = 0; m < M; m++) sel.push_back(m);
        return true;
    }
    int q = 0;
    bool pow4 = nmasks > 0;
    for (int64_t x = nmasks; pow4 && x > 1; x >>= 2, q++) pow4 = (x & 3) == 0;
    if (!pow4 || nmasks < 64) {
        err = "masks (" + std::to_string((long long)nmasks) + ") should be 0 (all masks) or a power of 4 that is >= 64";
        return false;
    }
    if (nmasks > M) {
        err = "masks (" + std::to_string((long long)nmasks) + ") should be <= the number of masks of the index (" + std::to_string(M) + ")";
        return false;
    }
    if (q > k) {
        err = "masks (" + std::to_string((long long)nmasks) + ") asks for a prefix of more bases than k = " + std::to_string(k);
        return false;
    }
    const int shift = (k - q) << 1;
    std::unordered_set<uint64_t> seen; // (the rule does not need sorted masks: "first in index order" of the prefixes met so far)
    for (int m = 0; m < M; m++)
        if (seen.insert(shift >= 64 ? 0 : masks[m] >> shift).second) sel.push_back(m);
    return true;
}

// pair.go:236: int(minMaskFraction * float64(totalMasks))
static inline int64_t pair_required(double min_mask_fraction, int64_t total) { return (int64_t)(min_mask_fraction * (double)total); }

// ---- pieces.  counts[s]: candidate tuples of selected mask s.  A piece is a run [s0, s1) of whole selected masks; the pieces
// cover [0, ns) without gaps (a run of masks without tuples joins a neighbour), so "masks not yet processed" behind a piece
// is ns - s1.  A piece takes masks while its tuples stay within `soft` and its key stays within 64 bits:
//   key = slot1 | slot2 | mask in piece | LCP,  2 * slot_bits + mask_bits + 6 <= 64
// where a one-mask piece has no mask bits.  It always takes one mask.  false when one mask alone has more than `hard` tuples
// (*bad = its number in the selection) or when two slots and the LCP alone do not fit (*bad = -1): nothing smaller can be cut.
struct PairPiece {
    int32_t s0, s1;
    int64_t tuples;
    int mask_bits;
};
static inline int pair_key_bits(int slot_bits, int mask_bits) { return 2 * slot_bits + mask_bits + LM_PAIR_LEN_BITS; }
static inline bool pair_pieces(const int64_t *counts, int32_t ns, int64_t soft, int64_t hard, int slot_bits, std::vector<PairPiece> &out,
                               int32_t *bad) {
    out.clear();
    if (pair_key_bits(slot_bits, 0) > 64) {
        if (bad) *bad = -1;
        return false;
    }
    const int spare = 64 - pair_key_bits(slot_bits, 0);
    const int64_t max_masks = spare >= 31 ? ((int64_t)1 << 31) - 1 : (int64_t)1 << spare;
    int64_t any = 0;
    for (int32_t s = 0; s < ns; s++) {
        if (counts[s] > hard) {
            if (bad) *bad = s;
            return false;
        }
        any += counts[s];
    }
    if (any == 0) return true; // nothing to emit: no piece
    PairPiece p{0, 0, 0, 0};
    for (int32_t s = 0; s < ns; s++) {
        const int64_t n = counts[s];
        if (s > p.s0 && ((p.tuples > 0 && n > 0 && p.tuples + n > soft) || s - p.s0 >= max_masks)) {
            p.s1 = s;
            p.mask_bits = pair_bits(p.s1 - p.s0);
            out.push_back(p);
            p = PairPiece{s, s, 0, 0};
        }
        p.tuples += n;
    }
    p.s1 = ns;
    p.mask_bits = pair_bits(p.s1 - p.s0);
    out.push_back(p);
    return true;
}

// ---- rows.  pair = slot1 << slot_bits | slot2 with slot1 < slot2, slots numbered in ascending key order.
struct PairRow {
    uint64_t pair;
    uint32_t n_masks, sum_prefix;
};
// table and partial: ascending by pair, a pair at most once in each.  A piece holds whole masks, so only sums meet
// (pair.go:286-291).  Then the exact prune: a pair stays only while n_masks so far + masks not yet processed >= required -
// one that cannot reach `required` any more is never reported, so dropping it changes no row.
static inline void pair_add_partials(const std::vector<PairRow> &table, const std::vector<PairRow> &partial, int64_t masks_left,
                                     int64_t required, std::vector<PairRow> &out) {
    out.clear();
    size_t a = 0, b = 0;
    while (a < table.size() || b < partial.size()) {
        PairRow r;
        if (b == partial.size() || (a < table.size() && table[a].pair < partial[b].pair)) {
            r = table[a++];
        } else if (a == table.size() || partial[b].pair < table[a].pair) {
            r = partial[b++];
        } else {
            r = table[a++];
            r.n_masks += partial[b].n_masks;
            r.sum_prefix += partial[b].sum_prefix;
            b++;
        }
        if ((int64_t)r.n_masks + masks_left >= required) out.push_back(r);
    }
}

// pair.go:995-1004: n_masks descending, sum_prefix descending, pair (= key1, key2) ascending
static inline bool pair_row_less(const PairRow &a, const PairRow &b) {
    if (a.n_masks != b.n_masks) return a.n_masks > b.n_masks;
    if (a.sum_prefix != b.sum_prefix) return a.sum_prefix > b.sum_prefix;
    return a.pair < b.pair;
}
static inline void pair_order(std::vector<PairRow> &rows) { std::sort(rows.begin(), rows.end(), pair_row_less); }

// pair.go:721, :730 (no newline).  Returns the length that was / would be written.
static inline const char *pair_header() { return "genome1\tgenome2\tminPrefix\tfracMasks\tnMasks\tsumPrefix\tavgPrefix"; }
static inline int pair_format_row(const char *genome1, const char *genome2, int min_prefix, uint32_t n_masks, uint32_t sum_prefix,
                                  int total_masks, char *buf, size_t cap) {
    char tail[160];
    const double frac = (double)n_masks / (double)total_masks, avg = (double)sum_prefix / (double)n_masks;
    char avg_s[48];
    if (std::isnan(avg)) snprintf(avg_s, sizeof avg_s, "NaN"); // (Go's %.2f of 0 / 0; no reported pair has n_masks == 0)
    else snprintf(avg_s, sizeof avg_s, "%.2f", avg);
    snprintf(tail, sizeof tail, "\t%d\t%.4f\t%u\t%u\t%s", min_prefix, frac, n_masks, sum_prefix, avg_s);
    const std::string line = std::string(genome1 ? genome1 : "") + "\t" + (genome2 ? genome2 : "") + tail;
    if (buf && cap) {
        const size_t n = std::min(line.size(), cap - 1);
        memcpy(buf, line.data(), n);
        buf[n] = 0;
    }
    return (int)line.size();
}

} // namespace lm
