// lm_residency.h — where the 2-bit genomes of a handle live: the device store (HBM) or pinned host memory (DESIGN.md
// §residency).  Host-only and free of HIP, so that the planner is tested without a device (tests/residency_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace lm {

// (values of lm_residency.genomes, include/lexicmap_hip.h)
enum { RES_GENOMES_AUTO = 0, RES_GENOMES_DEVICE = 1, RES_GENOMES_HOST = 2 };

// The device store keeps today's layout: a genome's bytes, then 8 .. 15 bytes of zero padding (the next genome starts at a
// multiple of 8; the 64-bit loads of the k-mer cutters may touch the word behind the last base).
static inline int64_t res_device_slot(int64_t nbytes) { return (nbytes + 15) & ~(int64_t)7; }
// A host-resident genome starts at a multiple of 16 of its pinned segment (k_stage_genome_bits loads 16 bytes per lane from
// 16-byte-aligned addresses) and has 16 .. 31 bytes of zero padding behind it: the last 16-byte load of a window that ends
// with the genome stays inside the genome's own slot.
#define LM_RES_HOST_ALIGN 16
static inline int64_t res_host_slot(int64_t nbytes) { return ((nbytes + 15) & ~(int64_t)15) + 16; }
// pinned segments of the host store: one allocation of hundreds of GB can fail where several smaller ones succeed
#define LM_RES_SEGMENT_BYTES ((int64_t)4 << 30)

struct GenomePlace {
    int32_t seg = -1; // -1: in the device store; else the pinned segment
    int64_t off = 0;  // byte offset of the genome's first byte in the device store / in its segment
};
struct ResidencyPlan {
    std::vector<GenomePlace> place;  // per local genome
    std::vector<int64_t> seg_bytes;  // size of every pinned segment
    int64_t genomes_device = 0, genomes_host = 0;
    int64_t bytes_device = 0, bytes_host = 0; // 2-bit bytes including the padding of each slot
};

// The split: genomes in local order go to the device while the byte budget lasts (slot sizes, padding included); the first
// genome that does not fit and every genome after it go to the host - a prefix on the device, a suffix on the host, so the
// split depends on nothing but the sizes and the budget.  A genome is never split, neither between the two places nor
// between two segments: a segment is closed when the next slot would take it past seg_cap (a slot larger than seg_cap gets
// a segment of its own).  mode DEVICE ignores the budget, mode HOST is a budget of 0.
static inline ResidencyPlan plan_residency(const std::vector<int64_t> &genome_bytes, int mode, int64_t budget, int64_t seg_cap) {
    ResidencyPlan p;
    p.place.resize(genome_bytes.size());
    if (seg_cap < 1) seg_cap = 1;
    bool spilled = mode == RES_GENOMES_HOST;
    for (size_t g = 0; g < genome_bytes.size(); g++) {
        const int64_t nb = genome_bytes[g] < 0 ? 0 : genome_bytes[g];
        if (!spilled && mode != RES_GENOMES_DEVICE && p.bytes_device + res_device_slot(nb) > budget) spilled = true;
        GenomePlace &pl = p.place[g];
        if (!spilled) {
            pl.seg = -1;
            pl.off = p.bytes_device;
            p.bytes_device += res_device_slot(nb);
            p.genomes_device++;
        } else {
            const int64_t slot = res_host_slot(nb);
            if (p.seg_bytes.empty() || p.seg_bytes.back() + slot > seg_cap) p.seg_bytes.push_back(0);
            pl.seg = (int32_t)p.seg_bytes.size() - 1;
            pl.off = p.seg_bytes.back();
            p.seg_bytes.back() += slot;
            p.bytes_host += slot;
            p.genomes_host++;
        }
    }
    return p;
}

// One staged chain window (k_stage_genome_bits): the bytes [first, first + copy) of a host-resident genome - from the byte
// that holds base tBegin, rounded down to 16, through the byte of the window's last base, rounded up to 16 - followed by 32
// bytes of zeros.  The k-mer cutters read at most 7 bytes before the first base's byte (aligned 64-bit words) and at most 20
// bytes past the last one's (kmer_from_bits' second word, the five-dword gather of k_pa_filter): both inside the range.
#define LM_STAGE_TAIL 32
struct StageRange {
    int64_t first = 0; // byte of the genome the copy starts at (multiple of 16)
    int64_t copy = 0;  // bytes copied from the host (multiple of 16)
    int64_t total() const { return copy + LM_STAGE_TAIL; }
};
static inline StageRange stage_range(int32_t tBegin, int32_t wlen) {
    StageRange r;
    r.first = ((int64_t)tBegin >> 2) & ~(int64_t)15;
    const int64_t last = (((int64_t)tBegin + wlen - 1) >> 2) + 1; // one past the byte of the window's last base
    r.copy = ((last - r.first) + 15) & ~(int64_t)15;
    return r;
}

} // namespace lm
