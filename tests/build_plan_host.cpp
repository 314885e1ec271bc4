// Host build of the genome builder's record planner (lexicmap_amd/csrc/lm_build_plan.h) for tests/test_build_plan_cpu.py.
#include "../lexicmap_amd/csrc/lm_build_plan.h"

using namespace lm;

extern "C" {

// plans one input genome of nc contigs; returns the number of records (first / n / len / bases per record, dst_off per contig)
// or -(BUILD_* reason) when the genome is refused
int bp_plan(const uint32_t *lens, int nc, int k, int interval, int64_t max_genome, int *first, int *n, int32_t *len, int64_t *bases,
            int32_t *dst_off) {
    std::vector<BuildRecord> recs;
    const int rc = plan_genome_records(lens, (size_t)nc, k, interval, max_genome, recs);
    if (rc != BUILD_OK) return -rc;
    for (size_t r = 0; r < recs.size(); r++) {
        first[r] = recs[r].first;
        n[r] = recs[r].n;
        len[r] = recs[r].len;
        bases[r] = recs[r].bases;
        for (int c = 0; c < recs[r].n; c++) dst_off[recs[r].first + c] = recs[r].dst_off[(size_t)c];
    }
    return (int)recs.size();
}
// skip regions of record `rec` of the same genome (contigs back to back in `ascii`); returns their number (at most cap are written)
int bp_regions(const uint8_t *ascii, const uint32_t *lens, int nc, int k, int interval, int64_t max_genome, int rec, int cap, int32_t *s,
               int32_t *e) {
    std::vector<BuildRecord> recs;
    if (plan_genome_records(lens, (size_t)nc, k, interval, max_genome, recs) != BUILD_OK || rec < 0 || rec >= (int)recs.size()) return -1;
    std::vector<const uint8_t *> seqs((size_t)nc);
    size_t at = 0;
    for (int c = 0; c < nc; c++) {
        seqs[(size_t)c] = ascii + at;
        at += lens[c];
    }
    std::vector<BuildRegion> regs;
    plan_skip_regions(recs[(size_t)rec], seqs.data(), lens, interval, regs);
    for (size_t i = 0; i < regs.size() && (int)i < cap; i++) {
        s[i] = regs[i].s;
        e[i] = regs[i].e;
    }
    return (int)regs.size();
}
uint64_t bp_key(int64_t n, int batch_size) { return build_genome_key(n, batch_size); }
int bp_keeps(int64_t first_record, int shard_count, int shard_rank) { return build_shard_keeps(first_record, shard_count, shard_rank) ? 1 : 0; }
unsigned bp_base_code(int c) { return build_base_code((uint8_t)c); }
int64_t bp_slot_bytes(int32_t len) { return build_slot_bytes(len); }
}
