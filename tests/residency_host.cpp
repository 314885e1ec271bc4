// Host build of the genome placement planner (lexicmap_amd/csrc/lm_residency.h) for tests/test_residency_plan_cpu.py.
#include "../lexicmap_amd/csrc/lm_residency.h"

using namespace lm;

extern "C" {

// plans `n` genomes of bytes[i] 2-bit bytes; per genome seg[i] (-1: device) and off[i]; seg_bytes_out[0 .. return value) the
// pinned segments (at most seg_cap_n of them are written); totals[4] = genomes on device / host, bytes on device / host
int rh_plan(const int64_t *bytes, int64_t n, int mode, int64_t budget, int64_t seg_cap, int32_t *seg, int64_t *off,
            int64_t *seg_bytes_out, int seg_cap_n, int64_t *totals) {
    std::vector<int64_t> b(bytes, bytes + n);
    const ResidencyPlan p = plan_residency(b, mode, budget, seg_cap);
    for (int64_t i = 0; i < n; i++) {
        seg[i] = p.place[(size_t)i].seg;
        off[i] = p.place[(size_t)i].off;
    }
    for (size_t i = 0; i < p.seg_bytes.size() && (int)i < seg_cap_n; i++) seg_bytes_out[i] = p.seg_bytes[i];
    totals[0] = p.genomes_device;
    totals[1] = p.genomes_host;
    totals[2] = p.bytes_device;
    totals[3] = p.bytes_host;
    return (int)p.seg_bytes.size();
}
int64_t rh_device_slot(int64_t nbytes) { return res_device_slot(nbytes); }
int64_t rh_host_slot(int64_t nbytes) { return res_host_slot(nbytes); }
// the staged byte range of a chain window: first copied byte, copied bytes, bytes taken in the staging buffer
void rh_stage_range(int32_t tbegin, int32_t wlen, int64_t *out) {
    const StageRange r = stage_range(tbegin, wlen);
    out[0] = r.first;
    out[1] = r.copy;
    out[2] = r.total();
}
}
