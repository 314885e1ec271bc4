// lm_build_plan.h — the record planner of the genome builder (lm_index_builder_*, lm_builder.hip): which contigs of an input
// genome form which genome record, where every contig and spacer lies in the record's concatenation, which stretches no seed
// may touch, and which key / shard a record gets.  Host-only and free of HIP, so that it is tested without a device
// (tests/build_plan_host.cpp).  The rules are the reference builder's (lib-index-build.go), each cited where it is applied.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace lm {

// genome/genome.go:1427-1444: A 0, C 1, G 2, T/U 3; of the ambiguity codes B, S and Y give 1 and K gives 2; everything else,
// N included, gives 0.  Lower case counts as upper case.
#if defined(__HIPCC__)
__host__ __device__
#endif
static inline uint32_t build_base_code(uint8_t c) {
    switch (c & 0xDFu) {
    case 'C': case 'B': case 'S': case 'Y': return 1;
    case 'G': case 'K': return 2;
    case 'T': case 'U': return 3;
    default: return 0;
    }
}

struct BuildRegion {
    int32_t s, e; // inclusive, in the record's concatenation
};

// One genome record: contigs [first, first + n) of the input genome joined with `interval` A's.
struct BuildRecord {
    int first = 0, n = 0;
    int32_t len = 0;              // bases of the concatenation, spacers included
    int64_t bases = 0;            // sum of the contig lengths (genome_size of the record)
    std::vector<int32_t> dst_off; // [n] where every contig starts in the concatenation
};

enum { BUILD_OK = 0, BUILD_NO_CONTIG = 1, BUILD_BIG_CONTIG = 2, BUILD_SHORT = 3, BUILD_LONG = 4 };

// lib-index-build.go:1581-1658: contigs are appended while the concatenation, spacers included, stays within max_genome; a
// contig that would overflow it closes the record and starts the next chunk of the same genome.  A genome with one contig
// longer than max_genome is skipped as a whole ("skipping a big genome"), and so is - here: before anything of it is added -
// a genome one of whose records is shorter than k or has 2^28 bases or more.  max_genome <= 0: 2^28 - 1.
static inline int plan_genome_records(const uint32_t *lens, size_t nc, int k, int interval, int64_t max_genome, std::vector<BuildRecord> &out) {
    out.clear();
    if (nc == 0) return BUILD_NO_CONTIG;
    const int64_t maxg = max_genome > 0 ? max_genome : ((int64_t)1 << 28) - 1;
    for (size_t i = 0; i < nc; i++)
        if ((int64_t)lens[i] > maxg) return BUILD_BIG_CONTIG;
    size_t first = 0;
    int64_t cur = 0;
    auto close = [&](size_t end) {
        BuildRecord r;
        r.first = (int)first;
        r.n = (int)(end - first);
        int64_t at = 0;
        for (size_t i = first; i < end; i++) {
            if (i > first) at += interval;
            r.dst_off.push_back((int32_t)(at & 0x7fffffff));
            at += lens[i];
            r.bases += lens[i];
        }
        const int rc = at < k ? BUILD_SHORT : at >= ((int64_t)1 << 28) ? BUILD_LONG : BUILD_OK;
        r.len = (int32_t)(at & 0x7fffffff);
        out.push_back(std::move(r));
        return rc;
    };
    int rc = BUILD_OK;
    for (size_t i = 0; i < nc && rc == BUILD_OK; i++) {
        if (cur + (int64_t)lens[i] > maxg && i > first) {
            rc = close(i);
            first = i;
            cur = 0;
        }
        if (i > first) cur += interval;
        cur += lens[i];
    }
    if (rc == BUILD_OK) rc = close(nc);
    if (rc != BUILD_OK) out.clear();
    return rc;
}

// The stretches of a record no seed may touch, ascending and disjoint (lib-index-build.go:971-1016): every spacer, and every
// run of at least 5 N / n (lib-gaps.go:38-60; a shorter run is stored as A's and seeded like any other bases).  A k-mer that
// overlaps a region is never captured and never fills a seed desert: its start lies in [s - k + 1, e].
// seqs / lens: the contigs of the whole input genome (the record names its own by first / n).
static inline void plan_skip_regions(const BuildRecord &r, const uint8_t *const *seqs, const uint32_t *lens, int interval, std::vector<BuildRegion> &out) {
    out.clear();
    for (int c = 0; c < r.n; c++) {
        const int32_t at = r.dst_off[(size_t)c];
        if (c > 0) out.push_back(BuildRegion{at - interval, at - 1});
        const uint8_t *s = seqs[r.first + c];
        const uint32_t n = lens[r.first + c];
        for (uint32_t i = 0; i < n;) {
            if (s[i] != 'N' && s[i] != 'n') {
                i++;
                continue;
            }
            const uint32_t st = i++;
            while (i < n && (s[i] == 'N' || s[i] == 'n')) i++;
            if (i - st >= 5) out.push_back(BuildRegion{at + (int32_t)st, at + (int32_t)i - 1});
        }
    }
}

// key of genome record number n (genomes.map.bin, the seed values): batch << 17 | index in the batch
static inline uint64_t build_genome_key(int64_t n, int batch_size) {
    return ((uint64_t)(n / batch_size) << 17) | (uint64_t)(n % batch_size);
}
// the loader's rule (lm_format.h): the records of a genome live on the shard (dense number of its FIRST record) % shard_count
static inline bool build_shard_keeps(int64_t first_record, int shard_count, int shard_rank) {
    return shard_count <= 1 || (int)(first_record % shard_count) == shard_rank;
}
// device slot of a record's 2-bit bytes: starts on an 8-byte boundary, at least 16 bytes of zero padding behind the last base
static inline int64_t build_slot_bytes(int32_t len) { return ((((int64_t)len + 3) >> 2) + 16 + 7) & ~(int64_t)7; }

} // namespace lm
