// lm_subseq_plan.h — the host's part of lm_index_subseqs / lm_index_subseq_rows / lm_index_genome_seqs (lm_subseq.hip;
// DESIGN.md section 11): the rule of `lexicmap utils subseq` (lexicmap/cmd/subseq.go, genome/genome.go SubSeq / SubSeq2) - flanks,
// the clamps of the contig form and of the concatenated form, the resolution of a genome id and a contig id over the records
// of a split genome, the status of every region and the refusals of a call - the layout of the base blob, its cut into
// pieces, and the FASTA formatter.  Free of HIP, so that it is tested without a device (tests/subseq_plan_host.cpp) against
// the Python model (tests/subseq_model.py).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "lm_seed_walk.h"

namespace lm {

// (the values of LM_SUBSEQ_*, include/lexicmap_hip.h)
enum { SS_OK = 0, SS_NO_GENOME = 1, SS_NO_SEQ = 2, SS_OUT_OF_RANGE = 3, SS_NOT_LOCAL = 4 };
#define LM_SS_MAX_START ((int64_t)0xffffffff) /* what a region of the kernel holds (SsDevRegion, lm_subseq.hip): a 32-bit start in */
#define LM_SS_MAX_LEN ((int64_t)0x7fffffff)   /* the record and 31 bits of length; ss_plan refuses a region beyond either */
#define LM_SS_GROUP 16 /* output bases of one lane = bytes of one store; every region starts at a multiple of it in the blob */

// subseq.go:388-397, 569-578: the flanks swap on the '-' strand; eStart < 1 becomes 1, eEnd is clamped by the form
inline void ss_flanks(int64_t begin, int64_t end, bool rc, int64_t upstream, int64_t downstream, int64_t *e_start, int64_t *e_end) {
    *e_start = begin - (rc ? downstream : upstream);
    const int64_t behind = rc ? upstream : downstream;
    *e_end = end > INT64_MAX - behind ? INT64_MAX : end + behind; // (every form clamps it to a length)
    if (*e_start < 1) *e_start = 1;
}

// What is read of a record: `len` bases from 0-based position `src` of its concatenation; begin / end as reported (1-based,
// forward coordinates of the contig or of the concatenation).
struct SsWindow {
    int64_t src = 0, len = 0, begin = 0, end = 0;
    int32_t status = SS_OK;
};

// SubSeq2 (genome.go:1149-1426) for contig `ci` of a record: the contig's offset is the sum of the earlier contigs' sizes plus
// `interval` each; the bases are contig[e_start - 1 : min(e_end, seqLen)], none when e_start > seqLen; the reported end is
// min(e_end, seqLen).  A flank never runs into the spacer or the next contig.
inline SsWindow ss_contig_window(const int32_t *seq_sizes, int32_t ci, int32_t interval, int64_t e_start, int64_t e_end) {
    SsWindow w;
    int64_t off = 0;
    for (int32_t c = 0; c < ci; c++) off += (int64_t)seq_sizes[c] + interval;
    const int64_t seq_len = seq_sizes[ci];
    w.begin = e_start;
    w.end = e_end < seq_len ? e_end : seq_len;
    w.len = e_start > seq_len ? 0 : w.end - e_start + 1;
    w.src = off + e_start - 1;
    return w;
}

// SubSeq (genome.go:697-736) in the concatenated coordinates of a record of rec_len bases: clamped to [1, rec_len].  Two
// deviations: e_start beyond the record is SS_OUT_OF_RANGE (the reference reads past the record), and the clamped
// end is reported (the reference prints 0).
inline SsWindow ss_concat_window(int64_t rec_len, int64_t e_start, int64_t e_end) {
    SsWindow w;
    w.begin = e_start;
    w.end = e_end < rec_len ? e_end : rec_len;
    if (e_start > rec_len) {
        w.status = SS_OUT_OF_RANGE;
        return w;
    }
    w.len = w.end - e_start + 1;
    w.src = e_start - 1;
    return w;
}

// one record as the resolution sees it
struct SsRecView {
    const int32_t *seq_sizes = nullptr;
    const std::string *seq_ids = nullptr;
    int32_t nseqs = 0;
    int64_t len = 0;  // bases of the record's concatenation
    uint64_t key = 0; // batch << 17 | index
};
// the contig of a record with this id: its number, -1 none, -2 more than one (the reference adds the offset twice there,
// genome.go:1297-1308: refused, seq_idx is the unambiguous way to name such a contig)
inline int32_t ss_find_seq(const SsRecView &r, const char *seq_id) {
    int32_t at = -1;
    for (int32_t c = 0; c < r.nseqs; c++)
        if (r.seq_ids[c] == seq_id) {
            if (at >= 0) return -2;
            at = c;
        }
    return at;
}
struct SsResolved {
    int32_t rec = -1, seq_idx = -1, status = SS_OK;
};
// A region given by genome id (subseq.go:371, 403-423, 582-605): the genome's records in chunk order; the first record in which
// the contig id is found answers.  Without a contig id (seq_id null or ""): seq_idx >= 0 is that contig of the FIRST record,
// seq_idx < 0 the concatenated form of the first record (seq_idx stays -1).
inline SsResolved ss_resolve(const SsRecView *recs, int32_t nrecs, const char *seq_id, int32_t seq_idx) {
    SsResolved r;
    if (nrecs <= 0) {
        r.status = SS_NO_GENOME;
        return r;
    }
    if (!seq_id || !*seq_id) {
        r.rec = 0;
        if (seq_idx >= 0) {
            if (seq_idx >= recs[0].nseqs) r.status = SS_NO_SEQ;
            else r.seq_idx = seq_idx;
        }
        return r;
    }
    for (int32_t i = 0; i < nrecs; i++) {
        const int32_t f = ss_find_seq(recs[i], seq_id);
        if (f == -1) continue; // the sequence might not be in this genome chunk
        r.rec = i;
        if (f < 0) r.status = SS_NO_SEQ;
        else r.seq_idx = f;
        return r;
    }
    r.status = SS_NO_SEQ;
    return r;
}

inline const char *ss_status_text(int32_t st) {
    switch (st) {
    case SS_OK: return "ok";
    case SS_NO_GENOME: return "the genome is not in this index";
    case SS_NO_SEQ: return "the sequence is in none of the genome's records, or its id occurs twice in one record (name it by seq_idx)";
    case SS_OUT_OF_RANGE: return "the region begins behind the end of the record";
    case SS_NOT_LOCAL: return "the record belongs to another shard";
    }
    return "unknown status";
}

// ---- the plan of a call: every region against the handle's records, the refusals
#define LM_SS_BY_NAME (~(uint64_t)0) /* (LM_REGION_BY_NAME, include/lexicmap_hip.h) */
// (lm_region, include/lexicmap_hip.h)
struct SsRegion {
    uint64_t key = 0; // record key, or LM_SS_BY_NAME: genome_id is resolved
    const char *genome_id = nullptr, *seq_id = nullptr;
    int32_t seq_idx = -1, rc = 0;
    int64_t begin = 0, end = 0;
};
// what the plan asks of a handle (lm_subseq.hip: the resident index; tests/subseq_plan_host.cpp: a table)
struct SsLookup {
    virtual ~SsLookup() {}
    virtual int32_t local_of(uint64_t key) const = 0;                                // the local record with this key, -1: none
    virtual bool elsewhere(uint64_t key) const = 0;                                  // a record that another shard holds
    virtual const std::vector<int32_t> *records_of(const char *genome_id) const = 0; // its local records in chunk order; null: none
    virtual SsRecView record(int32_t local) const = 0;
};
// the plan of one region
struct SsItem {
    int32_t local = -1, seq_idx = -1, status = SS_OK, rc = 0;
    int32_t bad = 0; // refused with or without ignore_errors: 1: begin < 1, 2: end < begin (subseq.go:530-535), 3: beyond the kernel's fields
    uint64_t key = 0;
    SsWindow w;
};
inline void ss_plan_one(const SsLookup &L, int32_t interval, const SsRegion &rg, int64_t upstream, int64_t downstream, SsItem &it) {
    it = SsItem();
    it.rc = rg.rc != 0;
    if (rg.begin < 1) {
        it.bad = 1;
        return;
    }
    if (rg.end < rg.begin) {
        it.bad = 2;
        return;
    }
    int64_t es, ee;
    ss_flanks(rg.begin, rg.end, it.rc != 0, upstream, downstream, &es, &ee);
    it.w.begin = es;
    it.w.end = ee;
    if (rg.key == LM_SS_BY_NAME) {
        const std::vector<int32_t> *mine = rg.genome_id ? L.records_of(rg.genome_id) : nullptr;
        if (!mine || mine->empty()) {
            it.status = SS_NO_GENOME;
            return;
        }
        std::vector<SsRecView> recs;
        for (int32_t l : *mine) recs.push_back(L.record(l));
        const SsResolved r = ss_resolve(recs.data(), (int32_t)recs.size(), rg.seq_id, rg.seq_idx);
        if (r.rec >= 0) {
            it.local = (*mine)[(size_t)r.rec];
            it.key = recs[(size_t)r.rec].key;
        }
        it.status = r.status;
        it.seq_idx = r.seq_idx;
    } else {
        it.key = rg.key;
        it.local = L.local_of(rg.key);
        if (it.local < 0) {
            it.status = L.elsewhere(rg.key) ? SS_NOT_LOCAL : SS_NO_GENOME;
            return;
        }
        const SsRecView v = L.record(it.local);
        if (rg.seq_id && *rg.seq_id) {
            const int32_t c = ss_find_seq(v, rg.seq_id);
            if (c < 0) it.status = SS_NO_SEQ;
            else it.seq_idx = c;
        } else if (rg.seq_idx >= 0) {
            if (rg.seq_idx >= v.nseqs) it.status = SS_NO_SEQ;
            else it.seq_idx = rg.seq_idx;
        }
    }
    if (it.status != SS_OK) return;
    const SsRecView v = L.record(it.local);
    it.w = it.seq_idx >= 0 ? ss_contig_window(v.seq_sizes, it.seq_idx, interval, es, ee) : ss_concat_window(v.len, es, ee);
    it.status = it.w.status;
    if (it.status != SS_OK || it.w.len == 0) return; // (a region that begins behind its contig's end: answered, no bases, nothing is read)
    if (it.w.src < 0 || it.w.src + it.w.len > v.len) { // (a contig table that does not fit its record)
        it.status = SS_OUT_OF_RANGE;
        it.w.len = 0;
    } else if (it.w.src > LM_SS_MAX_START || it.w.len > LM_SS_MAX_LEN) {
        it.bad = 3;
    }
}
// The verdict on region i: false with the refusal's text - the region's number and what failed.  ignore_errors keeps a region
// that has a status; begin < 1, end < begin and a region beyond the kernel's fields are refused in either mode.
inline bool ss_plan_verdict(const char *who, size_t i, const SsRegion &rg, const SsItem &it, bool ignore_errors, std::string &err) {
    const std::string what = std::string(who) + ": region " + std::to_string(i);
    if (it.bad == 1) {
        err = what + ": both begin and end position should not be <= 0";
        return false;
    }
    if (it.bad == 2) {
        err = what + ": begin position should be <= end position";
        return false;
    }
    if (it.bad == 3) {
        err = what + ": a region of 2^31 bases or more, or one that starts behind base 2^32 of its record, is not supported";
        return false;
    }
    if (it.status == SS_OK || ignore_errors) return true;
    const std::string name = rg.key == LM_SS_BY_NAME ? std::string("genome ") + (rg.genome_id ? rg.genome_id : "(null)")
                                                     : "key " + std::to_string(rg.key) + " (batch " + std::to_string(rg.key >> 17) + ", index " + std::to_string(rg.key & 0x1ffff) + ")";
    const std::string seq = rg.seq_id && *rg.seq_id ? std::string(", sequence ") + rg.seq_id : rg.seq_idx >= 0 ? ", sequence number " + std::to_string(rg.seq_idx) : "";
    err = what + " (" + name + seq + ", " + std::to_string((long long)rg.begin) + "-" + std::to_string((long long)rg.end) + "): " + ss_status_text(it.status) +
          "; ignore_errors answers the other regions";
    return false;
}
// The regions get(0 .. n - 1) -> items; false with the text of the first refusal (LM_ERR_ARG: nothing is returned).  A region
// with a status keeps it and has no bases when ignore_errors is set.  par(n, f) runs f(a, b) over ranges that cover [0, n).
template <typename Get, typename Par>
inline bool ss_plan(const SsLookup &L, int32_t interval, const char *who, size_t n, Get get, int64_t upstream, int64_t downstream, bool ignore_errors,
                    std::vector<SsItem> &items, std::string &err, Par par) {
    if (upstream < 0 || downstream < 0) {
        err = std::string(who) + ": upstream and downstream should be >= 0";
        return false;
    }
    items.resize(n);
    par((int64_t)n, [&](int64_t a, int64_t b) {
        for (int64_t i = a; i < b; i++) ss_plan_one(L, interval, get((size_t)i), upstream, downstream, items[(size_t)i]);
    });
    for (size_t i = 0; i < n; i++) {
        if (!ss_plan_verdict(who, i, get(i), items[i], ignore_errors, err)) return false;
        if (items[i].status != SS_OK) items[i].w.len = 0;
    }
    return true;
}

// ---- layout: region i takes ceil(len / 16) groups of 16 bytes from group goff[i] on, i.e. from byte 16 goff[i] of the blob;
// goff has n + 1 entries, the last the total.  An empty region takes no group and shares its offset with its successor.
inline int64_t ss_layout(const int64_t *len, size_t n, int64_t *goff) {
    int64_t g = 0;
    for (size_t i = 0; i < n; i++) {
        goff[i] = g;
        g += (len[i] + LM_SS_GROUP - 1) / LM_SS_GROUP;
    }
    goff[n] = g;
    return g;
}
// A piece: the groups [g0, g1) of the blob - at most budget_bytes / 16 of them, at least one - and the regions [r0, r1) that
// own a group of it.  A region larger than a piece is cut at a multiple of 16 bases, between two lanes' groups.
struct SsPiece {
    int64_t g0 = 0, g1 = 0, r0 = 0, r1 = 0;
};
inline void ss_pieces(const int64_t *goff, size_t n, int64_t budget_bytes, std::vector<SsPiece> &out) {
    out.clear();
    const int64_t total = goff[n];
    int64_t per = budget_bytes / LM_SS_GROUP;
    if (per < 1) per = 1;
    for (int64_t g0 = 0; g0 < total; g0 += per) {
        SsPiece p;
        p.g0 = g0;
        p.g1 = g0 + per < total ? g0 + per : total;
        p.r0 = sw_last_le(goff, 0, (int64_t)n - 1, p.g0);
        p.r1 = sw_last_le(goff, p.r0, (int64_t)n - 1, p.g1 - 1) + 1;
        out.push_back(p);
    }
}

// ---- one lane of k_subseq_extract (lm_subseq.hip), here so that the host runs it too (tests/subseq_plan_host.cpp, under
// AddressSanitizer over a buffer that holds exactly the region's bytes)
// The bytes [b, b + 4) of the genome as one word, first byte in the top bits (src + b is a multiple of 4).  Only bytes inside
// [lo, hi] - the bytes that hold bases of the lane's region - are dereferenced; the others read as 0.
LM_SW_HD uint32_t ss_word(const uint8_t *src, int64_t b, int64_t lo, int64_t hi) {
    if (b >= lo && b + 3 <= hi) {
        uint32_t x;
        __builtin_memcpy(&x, __builtin_assume_aligned(src + b, 4), 4);
        return __builtin_bswap32(x);
    }
    uint32_t w = 0;
    for (int k = 0; k < 4; k++)
        if (b + k >= lo && b + k <= hi) w |= (uint32_t)src[b + k] << (24 - 8 * k);
    return w;
}
// The 16 output bytes from output base o0 (a multiple of 16, < len) of the region `len` bases from base `start` of the 2-bit
// genome at src (4 bases per byte, first base in bits 7-6), forward or - rc - reverse complement: "ACGT"[code], zero behind
// the region's last base; byte j of the group is bits 8 (j & 3) of w[j >> 2].
LM_SW_HD void ss_group(const uint8_t *src, int64_t start, int64_t len, bool rc, int64_t o0, uint32_t w[4]) {
    const int nb = (int)(len - o0 < LM_SS_GROUP ? len - o0 : LM_SS_GROUP);             // the group's bases: 1 .. 16
    const int64_t pmin = rc ? start + len - o0 - nb : start + o0, pmax = pmin + nb - 1; // their source positions
    const int64_t lo = start >> 2, hi = (start + len - 1) >> 2;                        // the region's bytes
    const uintptr_t s = (uintptr_t)src;
    const int64_t b0 = (int64_t)(((s + (uintptr_t)(pmin >> 2)) & ~(uintptr_t)3) - s);   // the aligned word of the first base (< 0: starts before src)
    uint64_t v = (uint64_t)ss_word(src, b0, lo, hi) << 32;
    if (b0 + 4 <= (pmax >> 2)) v |= ss_word(src, b0 + 4, lo, hi);
    const int rel = (int)(pmin - 4 * b0);                                               // 0 .. 15: the first base's place in v
    const uint32_t y = (uint32_t)((v << (2 * rel)) >> 32);                              // source base i at bits 31 - 2 i, 30 - 2 i
    w[0] = w[1] = w[2] = w[3] = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < LM_SS_GROUP; j++) {
        const int i = rc ? nb - 1 - j : j;
        uint32_t code = (y >> ((30 - 2 * i) & 31)) & 3u;
        if (rc) code = 3u - code;
        const uint32_t ch = j < nb ? (0x54474341u >> (8 * code)) & 0xffu : 0u;           // "ACGT"[code]
        w[j >> 2] |= ch << (8 * (j & 3));
    }
}

// ---- the FASTA text
// wrapByteSlice (util.go:311-347): lines of `width`, no newline behind the last one; width < 1: no wrapping
inline void ss_wrap(std::string &out, const char *s, int64_t n, int width) {
    if (width < 1 || n == 0) {
        out.append(s, (size_t)n);
        return;
    }
    for (int64_t at = 0; at < n; at += width) {
        if (at) out.push_back('\n');
        out.append(s + at, (size_t)(n - at < width ? n - at : width));
    }
}
// >%s:%d-%d:%s (subseq.go:632-636): `name` is the contig id, or the genome id in the concatenated form; with `row` - the TSV
// line of the search row (its first 20 columns, tab-separated) - the long header of subseq.go:204-205, 447-450 (no newline)
inline void ss_header(std::string &out, const char *name, int64_t begin, int64_t end, bool rc, const char *row) {
    char num[64];
    out.push_back('>');
    out.append(name ? name : "");
    snprintf(num, sizeof num, ":%lld-%lld:%c", (long long)begin, (long long)end, rc ? '-' : '+');
    out.append(num);
    if (!row) return;
    // columns: 0 query 1 qlen 2 hits 3 sgenome 4 sseqid 5 qcovGnm 6 cls 7 hsp 8 qcovHSP 9 alenHSP 10 pident 11 gaps 12 qstart 13 qend
    // 14 sstart 15 send 16 sstr 17 slen 18 evalue 19 bitscore
    static const char *const key[20] = {" query=", nullptr, nullptr, " sgenome=", " sseqid=", " qcovGnm=", " cls=", " hsp=", " qcovHSP=", " alenHSP=",
                                        " pident=", " gaps=", " qstart=", " qend=", " sstart=", " send=", " sstr=", " slen=", " evalue=", " bitscore="};
    const char *p = row;
    for (int c = 0; c < 20; c++) {
        const char *e = strchr(p, '\t');
        const size_t n = e ? (size_t)(e - p) : strlen(p);
        if (key[c]) {
            out.append(key[c]);
            out.append(p, n);
        }
        if (!e) break;
        p = e + 1;
    }
}

} // namespace lm
