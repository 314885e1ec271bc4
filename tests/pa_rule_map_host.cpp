// Host harness of the rule map of the pseudo-alignment filter (lm_pa_filter_preset / lm_pa_filter_set / lm_pa_candidate3,
// lm_algos.h): the filter of one k-mer set built the way k_build_cmp_bits builds it, the rule map held to the rule evaluated
// literally from the exact sets of 11-base and 9-base prefixes, and lm_pa_candidate3 held to lm_pa_candidate2 on random keys.
// Test infrastructure only (tests/test_pa_rule_map_cpu.py builds it into a shared object of its own, and - under the
// sanitizers - into the stand-alone program of tests/pa_rule_map_main.cpp).
#include "../lexicmap_amd/csrc/lm_algos.h"
#include <set>
#include <stdio.h>
#include <vector>

extern "C" unsigned long long rm_bits_words(int log) { return lm_pa_bits_words(log); }
extern "C" int rm_filter_log(long long nk) { return lm_pa_filter_log(nk); }

// what the host memset + k_build_cmp_bits do for one query: `bits` holds lm_pa_bits_words(log) zeroed words
extern "C" void rm_build(const uint64_t *keys, int n, int K, int log, uint32_t *bits) {
    auto or_bit = [&](uint64_t w, uint32_t m) { bits[w] |= m; };
    lm_pa_filter_preset(log, 0, 1, or_bit);
    for (int i = 0; i < n; i++) lm_pa_filter_set(keys[i], K, log, or_bit);
}

extern "C" int rm_candidate2(const uint32_t *bits, int log, uint32_t f, int p) {
    return lm_pa_candidate2(bits + lm_pa_bloom_word0(log), lm_pa_bloom_log(log), bits + lm_pa_map9_word0(log), bits, log, f, p);
}
extern "C" int rm_candidate3(const uint32_t *bits, int log, uint32_t f, int p) {
    return lm_pa_candidate3(bits + lm_pa_bloom_word0(log), lm_pa_bloom_log(log), bits + lm_pa_rule_word0(log), bits, log, f, p);
}

// the terms of the tests for a key of p bases, one bit each: 1 Bloom filter hit, 2 hashed 11-base bitmap hit, 4 bases [9, p) all
// A, 8 the rule-map bit of its first nine bases, 16 the 9-base map's
extern "C" int rm_parts(const uint32_t *bits, int log, uint32_t f, int p) {
    const int blog = lm_pa_bloom_log(log);
    const uint32_t *bloom = bits + lm_pa_bloom_word0(log);
    const uint32_t p11 = f >> ((p - 11) << 1), p9 = f >> ((p - 9) << 1);
    const uint32_t a = lm_pa_bloom_slot(p11, 0, blog), b = lm_pa_bloom_slot(p11, 1, blog), h = lm_pa_filter_slot(p11, log);
    int r = (int)((bloom[a >> 5] >> (a & 31)) & (bloom[b >> 5] >> (b & 31)) & 1u);
    r |= (int)((bits[h >> 5] >> (h & 31)) & 1u) << 1;
    r |= (f & ((1u << ((p - 9) << 1)) - 1u)) == 0 ? 4 : 0;
    r |= (int)((bits[lm_pa_rule_word0(log) + (p9 >> 5)] >> (p9 & 31)) & 1u) << 3;
    r |= (int)((bits[lm_pa_map9_word0(log) + (p9 >> 5)] >> (p9 & 31)) & 1u) << 4;
    return r;
}

// every one of the 2^18 bits of the rule map against the rule written out over the exact prefix sets; returns the number of
// set bits, or -1 - p9 of the first bit that differs
extern "C" long long rm_check_exhaustive(const uint64_t *keys, int n, int K, const uint32_t *bits, int log) {
    std::set<uint32_t> s11, s9;
    for (int i = 0; i < n; i++) {
        s11.insert((uint32_t)(keys[i] >> ((K - 11) << 1)));
        s9.insert((uint32_t)(keys[i] >> ((K - 9) << 1)));
    }
    const uint32_t *rule = bits + lm_pa_rule_word0(log);
    long long nset = 0;
    for (uint32_t p9 = 0; p9 < (1u << 18); p9++) {
        const bool base8_a = (p9 & 3u) == 0, base7_a = ((p9 >> 2) & 3u) == 0;
        bool want = base7_a && base8_a;
        want = want || (s9.count(p9) != 0 && base8_a);
        for (uint32_t sib = 1; sib < 4; sib++) want = want || s11.count((p9 << 4) | sib) != 0;
        const bool got = ((rule[p9 >> 5] >> (p9 & 31)) & 1u) != 0;
        if (got != want) return -1 - (long long)p9;
        nset += got;
    }
    return nset;
}

namespace {
uint64_t mix(uint64_t *s) { // splitmix64
    uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
} // namespace

// `nkeys` seeded keys of p bases: lm_pa_candidate3 must imply lm_pa_candidate2.  A quarter each: uniform; bases [9, p) all A;
// the same with the first nine bases of a k-mer of the set; the first 11 bases of a k-mer of the set (a Bloom hit).
// out[0] / out[1] = keys candidate2 / candidate3 let through; returns the number of keys candidate3 passes and candidate2 does not
extern "C" long long rm_no_growth(const uint64_t *keys, int n, int K, const uint32_t *bits, int log, int p, uint64_t seed,
                                  long long nkeys, long long *out) {
    long long bad = 0;
    out[0] = out[1] = 0;
    const uint32_t fmask = (1u << (2 * p)) - 1u, tail = (1u << ((p - 9) << 1)) - 1u;
    for (long long j = 0; j < nkeys; j++) {
        uint32_t f = (uint32_t)mix(&seed) & fmask;
        const int kind = (int)(j & 3);
        if (kind == 1) f &= ~tail;
        if (kind == 2 && n > 0) {
            uint32_t p9 = (uint32_t)(keys[mix(&seed) % (uint64_t)n] >> ((K - 9) << 1));
            if (j & 4) p9 ^= (uint32_t)mix(&seed) & 3u; // (every other one: base 8 varied)
            f = p9 << ((p - 9) << 1);
        }
        if (kind == 3 && n > 0) {
            const uint32_t p11 = (uint32_t)(keys[mix(&seed) % (uint64_t)n] >> ((K - 11) << 1));
            f = (p11 << ((p - 11) << 1)) | (f & ((1u << ((p - 11) << 1)) - 1u));
        }
        const bool c2 = rm_candidate2(bits, log, f, p) != 0, c3 = rm_candidate3(bits, log, f, p) != 0;
        out[0] += c2;
        out[1] += c3;
        bad += c3 && !c2;
    }
    return bad;
}
