// Host harness of the nested-anchor rule of the pseudo-alignment (lm_pa_anchor_nested, lm_algos.h): one chain window
// against one query, the way k_extract_kmers / k_pa_search see them, next to a plain model.  Test infrastructure only
// (tests/test_pa_nested_cpu.py builds it into a shared object of its own).
#include "../lexicmap_amd/csrc/lm_algos.h"
#include <algorithm>
#include <set>
#include <stdio.h>
#include <string>
#include <tuple>
#include <vector>

namespace {
struct Anchor {
    int q, len, t, rcs; // QBegin, length, TBegin, strand of the search
    int x, i;           // query position of the matched k-mer, window position
    bool nested;
};
char comp(char c) {
    switch (c | 0x20) {
    case 'a': return 'T';
    case 'c': return 'G';
    case 'g': return 'C';
    case 't': return 'A';
    default: return 'N';
    }
}
uint64_t enc(const char *s, int k) {
    uint64_t c = 0;
    for (int j = 0; j < k; j++) c = (c << 2) | lm_base2bit((uint8_t)s[j]);
    return c;
}
int fail(char *err, int cap, const std::string &m) {
    snprintf(err, (size_t)cap, "%s", m.c_str());
    return 1;
}
} // namespace

enum { // counters
    C_RAW, C_NESTED, C_CLEARED, C_FWD_NESTED, C_REV_NESTED,
    C_WIN_POS0,   // forward anchors at window position 0 that only condition 2 keeps
    C_QBEGIN,     // forward anchors at the task's QBegin that only condition 6 keeps
    C_REV_LAST,   // reverse anchors at the last window position that only condition 2 keeps
    C_RUN31, C_RUN32, C_RUN40, // anchors of exact runs of 31, 32, 40 bases
    C_LP_P1,      // the predicate asked at lp + 1 == p and answering "nested" (the container is the anchor in hand)
    C_Q_LOWC,     // anchors that only condition 5 keeps (neighbouring query k-mer dropped from the index)
    C_Q_N,        // anchors whose neighbouring query base is an N
    C_QUIRK,      // anchors of the partial-prefix rule (shorter than p)
    C_NO_PREV,    // anchors kept because the window base is not in the two words
    C_LEN_K,      // anchors of full length K (never nested: lp < K)
    C_N
};

extern "C" int pn_ncounters() { return C_N; }

// genome g[0, glen) (ACGT), window = g[tbegin, tbegin + wlen) or its reverse complement (wrc); query q (may hold N);
// index_k != K: the comparison index is written twice, as stage_kmers does for an index whose k is not the comparison's
extern "C" int pn_case(const char *q, int qlen, const char *g, int glen, int tbegin, int wlen, int wrc, int K, int index_k, int p,
                       int qb, int qe, long long *cnt, char *err, int errcap) {
    // ---- the comparison index (k_extract_kmers + the segmented sort)
    const int npos = qlen - K + 1;
    if (npos <= 0 || wlen < K || tbegin < 0 || tbegin + wlen > glen) return fail(err, errcap, "bad case");
    std::vector<uint64_t> kc((size_t)2 * std::max(npos, qlen), 1ull << 63);
    std::vector<uint32_t> vc(kc.size(), 0u);
    std::vector<char> indexed((size_t)npos, 0);
    for (int pass = 0; pass < 2; pass++) {
        const int k = pass == 0 ? index_k : K;
        if (pass == 1 && index_k == K) break;
        const int np = qlen - k + 1;
        for (int x = 0; x < np; x++) {
            const uint64_t fwd = enc(q + x, k), rc = lm_revcomp(fwd, k);
            const bool filtered = fwd == 0 || lm_low_complexity(fwd, k);
            kc[2 * x] = filtered ? (1ull << 63) : fwd;
            kc[2 * x + 1] = filtered ? (1ull << 63) : rc;
            lm_cmp_vals((const uint8_t *)q, x, np, k, fwd, &vc[2 * x], &vc[2 * x + 1]);
            if (k == K) indexed[x] = !filtered;
        }
    }
    std::vector<uint32_t> val_of(vc.begin(), vc.begin() + 2 * npos); // by position and strand
    std::vector<int> ord((size_t)2 * npos);
    for (int j = 0; j < 2 * npos; j++) ord[j] = j;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return kc[a] < kc[b]; });
    std::vector<uint64_t> keys;
    std::vector<uint32_t> vals;
    for (int j : ord)
        if (kc[j] != (1ull << 63)) {
            keys.push_back(kc[j]);
            vals.push_back(vc[j]);
        }
    const int n = (int)keys.size();
    keys.push_back(1ull << 63);
    const int tab_bits = 12;
    std::vector<uint32_t> tab(((size_t)1 << tab_bits) + 1);
    for (uint32_t b = 0; b <= (1u << tab_bits); b++)
        tab[b] = b == (1u << tab_bits) ? (uint32_t)n : (uint32_t)lm_lower_bound_u64(keys.data(), 0, n, (uint64_t)b << ((K << 1) - tab_bits));
    // ---- the window, as text (plain) and as the packed genome the kernel reads
    std::string W(g + tbegin, g + tbegin + wlen);
    if (wrc) {
        std::reverse(W.begin(), W.end());
        for (char &c : W) c = comp(c);
    }
    std::vector<uint64_t> bits64((size_t)glen / 32 + 4, 0ull);
    uint8_t *gbits = (uint8_t *)bits64.data();
    for (int j = 0; j < glen; j++) gbits[j >> 2] |= (uint8_t)(lm_base2bit((uint8_t)g[j]) << (6 - 2 * (j & 3)));
    const int wnpos = wlen - K + 1;
    // ---- raw anchors: the plain model (every indexed query k-mer sharing >= p bases, then the range test), the kernel's
    // search beside it (they must agree), and the anchors of the partial-prefix rule from the kernel's search alone
    std::vector<Anchor> raw;
    for (int i = 0; i < wnpos; i++) {
        uint64_t kmer, rc;
        int wprev, wnext;
        lm_kmer_nb_from_bits(gbits, 0, wrc ? tbegin + wlen - K - i : tbegin + i, K, wrc != 0, &kmer, &rc, &wprev, &wnext);
        if (kmer != enc(W.data() + i, K) || rc != lm_revcomp(kmer, K)) return fail(err, errcap, "window k-mer from the packed genome differs from the text");
        if (wprev >= 0 && i >= 1 && wprev != (int)lm_base2bit((uint8_t)W[i - 1])) return fail(err, errcap, "window base i-1 differs from the text");
        if (wnext >= 0 && i + K < wlen && wnext != (int)lm_base2bit((uint8_t)W[i + K])) return fail(err, errcap, "window base i+K differs from the text");
        if (kmer == 0 || kmer == lm_ns(1, K) || kmer == lm_ns(2, K) || kmer == lm_kmer_mask(K)) continue;
        for (int rcs = 0; rcs < 2; rcs++) {
            const uint64_t key = rcs ? rc : kmer;
            const int nb = lm_pa_nested_window(rcs != 0, K, i, wnpos, kmer, rcs ? wnext : wprev);
            int lo = 0, hi = 0;
            uint64_t right = 0;
            const int r = lm_tree_search_first_tab(keys.data(), n, key, p, K, tab.data(), tab_bits, &lo, &hi, &right);
            std::vector<int> found; // indexes into keys
            for (int j = lo; r != 0 && j < hi && keys[j] <= right; j++) found.push_back(j);
            std::vector<int> plain;
            for (int j = 0; j < n; j++)
                if (lm_lcp(keys[j], key, K) >= p) plain.push_back(j);
            if (r == 1 ? plain != found : !plain.empty()) return fail(err, errcap, "the search and the plain model disagree");
            for (int j : found) {
                const uint32_t v = vals[j];
                const int x = (int)((v & LM_CMP_POS_MASK) >> 1), lp = lm_lcp(keys[j], key, K);
                if (v != val_of[2 * x + (v & 1u)]) return fail(err, errcap, "index value moved");
                Anchor a;
                a.rcs = rcs;
                a.x = x;
                a.i = i;
                a.len = lp;
                if (!rcs) {
                    a.q = x;
                    a.t = i;
                    if ((v & 1u) == 1u || a.q < qb || a.q + lp > qe) continue;
                } else {
                    a.q = x + K - lp;
                    a.t = i + K - lp;
                    if ((v & 1u) == 0u || a.q + lp < qb || a.q > qe) continue;
                }
                const uint32_t qnb = v >> LM_CMP_NB_SHIFT;
                const int wb = rcs ? wnext : wprev;
                a.nested = lm_pa_anchor_nested(rcs != 0, K, p, lp, i, wnpos, kmer, wb, qnb, a.q, qb);
                if (a.nested != lm_pa_nested_match(rcs != 0, K, p, lp, nb, qnb, a.q, qb)) return fail(err, errcap, "the two halves differ from the whole");
                raw.push_back(a);
                // ---- shapes
                if (r == 2) cnt[C_QUIRK]++;
                if (lp == K) cnt[C_LEN_K]++;
                if (wb < 0) cnt[C_NO_PREV]++;
                if (!a.nested) {
                    if (!rcs && i == 0 && wb >= 0 && lm_pa_anchor_nested(false, K, p, lp, 1, wnpos + 1, kmer, wb, qnb, a.q, qb)) cnt[C_WIN_POS0]++;
                    if (!rcs && a.q == qb && lm_pa_anchor_nested(false, K, p, lp, i, wnpos, kmer, wb, qnb, a.q, qb - 1)) cnt[C_QBEGIN]++;
                    if (rcs && i == wnpos - 1 && wb >= 0 && lm_pa_anchor_nested(true, K, p, lp, i, wnpos + 1, kmer, wb, qnb, a.q, qb)) cnt[C_REV_LAST]++;
                    if (!(qnb & 1u) && lm_pa_anchor_nested(rcs != 0, K, p, lp, i, wnpos, kmer, wb, qnb | 1u, a.q, qb)) cnt[C_Q_LOWC]++;
                }
                if (!rcs ? (x >= 1 && (q[x - 1] | 0x20) == 'n') : (x + K < qlen && (q[x + K] | 0x20) == 'n')) cnt[C_Q_N]++;
                { // the exact run the anchor lies in (forward: along the diagonal in the text; reverse: query against the complement)
                    int l = 0, rr = 0;
                    if (!rcs) {
                        while (a.q - 1 - l >= 0 && a.t - 1 - l >= 0 && lm_base2bit((uint8_t)q[a.q - 1 - l]) == lm_base2bit((uint8_t)W[a.t - 1 - l])) l++;
                        while (a.q + rr < qlen && a.t + rr < wlen && lm_base2bit((uint8_t)q[a.q + rr]) == lm_base2bit((uint8_t)W[a.t + rr])) rr++;
                        const int R = l + rr;
                        if (R == 31) cnt[C_RUN31]++;
                        if (R == 32) cnt[C_RUN32]++;
                        if (R == 40) cnt[C_RUN40]++;
                    }
                }
                // the predicate at lp + 1 == p: the anchor one position further into the run would have p - 1 bases; it is not in
                // the list (the normal rule needs p, the partial-prefix rule returns less than p - 1), and were it there, the
                // anchor in hand (length p, found by the normal rule) is its container
                if (r == 1 && lp == p && lp < K) {
                    const int i2 = rcs ? i - 1 : i + 1, x2 = rcs ? x - 1 : x + 1;
                    if (i2 >= 0 && i2 < wnpos && x2 >= 0 && x2 < npos && indexed[x2]) {
                        const uint64_t k2 = enc(W.data() + i2, K);
                        const int wb2 = (int)lm_base2bit((uint8_t)(rcs ? W[i2 + K] : W[i2 - 1]));
                        const int q2 = rcs ? a.q : a.q + 1;
                        if (lm_lcp(rcs ? lm_revcomp(k2, K) : k2, rcs ? lm_revcomp(enc(q + x2, K), K) : enc(q + x2, K), K) != p - 1)
                            return fail(err, errcap, "the neighbour inside the run is not one base shorter");
                        if (lm_pa_anchor_nested(rcs != 0, K, p, p - 1, i2, wnpos, k2, wb2, val_of[2 * x2 + rcs] >> LM_CMP_NB_SHIFT, q2, qb)) cnt[C_LP_P1]++;
                    }
                }
            }
        }
    }
    // ---- 1. every nested anchor has its container in the raw list
    std::set<std::tuple<int, int, int, int>> have;
    for (const Anchor &a : raw) have.insert(std::make_tuple(a.q, a.len, a.t, a.rcs));
    for (const Anchor &a : raw) {
        if (!a.nested) continue;
        const auto c = a.rcs ? std::make_tuple(a.q, a.len + 1, a.t, 1) : std::make_tuple(a.q - 1, a.len + 1, a.t - 1, 0);
        if (!have.count(c)) {
            char m[200];
            snprintf(m, sizeof m, "nested anchor (q %d, len %d, t %d, strand %d) has no container in the raw list", a.q, a.len, a.t, a.rcs);
            return fail(err, errcap, m);
        }
        cnt[a.rcs ? C_REV_NESTED : C_FWD_NESTED]++;
    }
    // ---- 2. ClearSubstrPairs over the raw list == over the list without the nested anchors, element for element
    std::vector<uint64_t> all, kept;
    for (const Anchor &a : raw) {
        const uint64_t k = lm_pack_anchor(a.q, a.len, a.t, a.rcs != 0, a.rcs != 0);
        all.push_back(k);
        if (!a.nested) kept.push_back(k);
    }
    std::sort(all.begin(), all.end());
    std::sort(kept.begin(), kept.end());
    auto clear = [&](const std::vector<uint64_t> &ks) {
        std::vector<LmSub> s;
        for (uint64_t k : ks) s.push_back(lm_unpack_anchor(k));
        std::vector<uint8_t> marks(s.size() + 1);
        const int m = lm_clear_sorted(s.data(), (int)s.size(), K, marks.data());
        s.resize((size_t)m);
        return s;
    };
    const std::vector<LmSub> ca = clear(all), ck = clear(kept);
    if (ca.size() != ck.size()) {
        char m[200];
        snprintf(m, sizeof m, "ClearSubstrPairs keeps %zu of %zu raw anchors but %zu of the %zu without the nested ones", ca.size(), all.size(),
                 ck.size(), kept.size());
        return fail(err, errcap, m);
    }
    for (size_t j = 0; j < ca.size(); j++)
        if (ca[j].qbegin != ck[j].qbegin || ca[j].tbegin != ck[j].tbegin || ca[j].len != ck[j].len || ca[j].qrc != ck[j].qrc || ca[j].trc != ck[j].trc)
            return fail(err, errcap, "ClearSubstrPairs results differ at element " + std::to_string(j));
    cnt[C_RAW] += (long long)all.size();
    cnt[C_NESTED] += (long long)(all.size() - kept.size());
    cnt[C_CLEARED] += (long long)ca.size();
    return 0;
}
