// lm_screen_plan.h — the host's part of genome screening (lm_screen.hip, lm_index_screen_genomes): how a query genome is
// laid out and cut into windows, how the tuples of a batch are cut into pieces, and how per-record sums become rows.
// Host-only and free of HIP, so that tests/screen_plan_host.cpp can hold it to the Python model (tests/screen_model.py).
// Reference: GSearchScreen, lib-index-search-genome.go:114-543; the query genome, search-genome-util.go:129-217.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

namespace lm {

// ---- the query genome (search-genome-util.go:155-182): contigs joined by k skipped bases; the skip regions are exactly
// those spacers, [s, s + k - 1] (N became A before anything looked for a gap, so a run of N is none)
struct ScreenLayout {
    int64_t len = 0;
    std::vector<int64_t> start;       // [ncontigs] where each contig begins in the concatenation
    std::vector<int32_t> reg_s, reg_e; // [ncontigs - 1] inclusive
};
static inline void screen_layout(const uint32_t *contig_len, size_t ncontigs, int k, ScreenLayout &out) {
    out = ScreenLayout();
    for (size_t c = 0; c < ncontigs; c++) {
        if (c > 0) {
            if (out.len < ((int64_t)1 << 31)) { // (a query this long is refused by the caller; the regions are then not used)
                out.reg_s.push_back((int32_t)out.len);
                out.reg_e.push_back((int32_t)(out.len + k - 1));
            }
            out.len += k;
        }
        out.start.push_back(out.len);
        out.len += contig_len[c];
    }
}

// ---- windows (lib-index-search-genome.go:150-173): step = len / (windows + 1), window = 2 * step (len when windows == 1),
// window i = [i * step, i * step + window), the last one runs to len.  Every window is there, also an empty one and one
// shorter than k (more windows than len / k): such a window holds no k-mer and captures nothing.
struct ScreenWindow {
    int64_t start, len;
};
static inline void screen_windows(int64_t len, int windows, std::vector<ScreenWindow> &out) {
    out.clear();
    const int64_t step = len / ((int64_t)windows + 1);
    const int64_t window = windows == 1 ? len : step * 2;
    for (int i = 0; i < windows; i++) {
        const int64_t s = (int64_t)i * step;
        const int64_t e = i == windows - 1 ? len : s + window;
        out.push_back(ScreenWindow{s, e - s});
    }
}

// ---- pieces.  The lookups are sorted by mask, so the tuples of masks [m0, m1) are one contiguous range of the emit order and
// every (query, record, mask) group lies inside one piece; a (query, record) group is spread over pieces and its partial sums
// are added up (screen_merge_partials).  A piece takes masks while it stays within `soft` tuples, but always one; false when
// one mask alone has more than `hard` tuples (*bad = that mask): nothing smaller can be cut.
struct ScreenPiece {
    int m0, m1;
    int64_t tuples;
};
static inline bool screen_pieces(const uint64_t *per_mask, int M, int64_t soft, int64_t hard, std::vector<ScreenPiece> &out, int *bad) {
    out.clear();
    ScreenPiece p{0, 0, 0};
    for (int m = 0; m < M; m++) {
        const int64_t n = (int64_t)per_mask[m];
        if (n > hard) {
            if (bad) *bad = m;
            return false;
        }
        if (p.tuples > 0 && p.tuples + n > soft) {
            p.m1 = m;
            out.push_back(p);
            p = ScreenPiece{m, m, 0};
        }
        p.tuples += n;
    }
    p.m1 = M;
    if (p.tuples > 0) out.push_back(p);
    return true;
}

// ---- sums of one (query, subject record).  A piece gives partial sums over its masks; pref_* names the Longest values of
// the piece's hit masks, in mask order, in the caller's byte store.
struct ScreenPartial {
    uint32_t query;
    int64_t local;       // the record's local number on this handle
    uint64_t score, score2, hit_kmers;
    uint32_t hit_masks;
    uint64_t pref_off;   // hit_masks bytes
};
// partial sums in any order -> one entry per (query, record), ascending; `chain[i]` lists the entries of `in` that made
// out[i] in piece order (their prefix bytes concatenated are the record's)
static inline void screen_merge_partials(const std::vector<ScreenPartial> &in, std::vector<ScreenPartial> &out,
                                         std::vector<std::vector<size_t>> &chain) {
    std::vector<size_t> ord(in.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
        if (in[a].query != in[b].query) return in[a].query < in[b].query;
        return in[a].local < in[b].local;
    });
    out.clear();
    chain.clear();
    for (size_t i : ord) {
        const ScreenPartial &p = in[i];
        if (out.empty() || out.back().query != p.query || out.back().local != p.local) {
            out.push_back(p);
            chain.emplace_back(1, i);
            continue;
        }
        ScreenPartial &o = out.back();
        o.score += p.score;
        o.score2 += p.score2;
        o.hit_kmers += p.hit_kmers;
        o.hit_masks += p.hit_masks;
        chain.back().push_back(i);
    }
}

// ---- rows (lib-index-search-genome.go:423-509).  One hit record: its key, the chunk list it belongs to (-1: the genome
// was not split) and its score.  Records of one list become one row: score summed, keys ascending, details of the record
// with the lowest key (the reference: whichever a Go map yields first).  Rows of a query: score descending, ties by
// ascending lowest key (the reference: an unstable sort), cut to top_n (0: all); queries in ascending order.
struct ScreenHit {
    uint32_t query;
    uint64_t key;
    int32_t list;
    uint64_t score;
};
struct ScreenRow {
    uint32_t query;
    uint64_t score;
    size_t detail;              // index into the hits: the record whose details the row carries
    std::vector<uint64_t> keys; // ascending; keys[0] is the row's key
};
static inline void screen_rows(const std::vector<ScreenHit> &hits, int top_n, std::vector<ScreenRow> &out) {
    std::vector<size_t> ord(hits.size());
    for (size_t i = 0; i < ord.size(); i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
        if (hits[a].query != hits[b].query) return hits[a].query < hits[b].query;
        return hits[a].key < hits[b].key;
    });
    out.clear();
    size_t i = 0;
    while (i < ord.size()) {
        const uint32_t q = hits[ord[i]].query;
        std::vector<ScreenRow> rows;
        std::unordered_map<int32_t, size_t> row_of_list;
        for (; i < ord.size() && hits[ord[i]].query == q; i++) {
            const ScreenHit &h = hits[ord[i]];
            ScreenRow *into = nullptr;
            if (h.list >= 0) {
                const auto it = row_of_list.find(h.list);
                if (it != row_of_list.end()) into = &rows[it->second];
                else row_of_list[h.list] = rows.size();
            }
            if (into) { // (keys come in ascending order: the first record of a list is its lowest)
                into->score += h.score;
                into->keys.push_back(h.key);
            } else {
                rows.push_back(ScreenRow{q, h.score, ord[i], std::vector<uint64_t>(1, h.key)});
            }
        }
        std::stable_sort(rows.begin(), rows.end(), [](const ScreenRow &a, const ScreenRow &b) {
            if (a.score != b.score) return a.score > b.score;
            return a.keys[0] < b.keys[0];
        });
        if (top_n > 0 && rows.size() > (size_t)top_n) rows.resize((size_t)top_n);
        for (ScreenRow &r : rows) out.push_back(std::move(r));
    }
}

} // namespace lm
