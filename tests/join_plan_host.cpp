// Host build of the record planner of lm_index_builder_add_index (lexicmap_amd/csrc/lm_join_plan.h) for
// tests/test_join_plan_cpu.py.
#include "../lexicmap_amd/csrc/lm_join_plan.h"

#include <string.h>

using namespace lm;

extern "C" {

// The source's record table: key / list (-1: not split) / list_n / list_idx per record, n records.  keep == NULL (has_keep
// == 0): every record.  Returns JOIN_OK (0) or the reason; err (cap bytes) gets the text.  new_bg: [n]; of the kept records
// (at most n, their number in *nkept): place in the source, record number, key, list, list_n, list_idx.
int jp_plan(const uint64_t *key, const int *list, const int *list_n, const int *list_idx, int n, int has_keep, const uint64_t *keep, int nkeep,
            int64_t next_record, int batch_size, int next_list, uint64_t *new_bg, int *nkept, int64_t *k_src, int64_t *k_number, uint64_t *k_key,
            int *k_list, int *k_list_n, int *k_list_idx, int64_t *ninput, int *nlists, int *drops, char *err, int cap) {
    std::vector<JoinSrcRecord> src((size_t)n);
    for (int i = 0; i < n; i++) {
        src[(size_t)i].key = key[i];
        src[(size_t)i].list = list[i];
        src[(size_t)i].list_n = list_n[i];
        src[(size_t)i].list_idx = list_idx[i];
    }
    static const uint64_t none = 0;
    JoinPlan p;
    std::string e;
    const int rc = plan_join(src, has_keep ? (keep ? keep : &none) : nullptr, (size_t)nkeep, next_record, batch_size, next_list, p, e);
    if (cap > 0) {
        strncpy(err, e.c_str(), (size_t)cap - 1);
        err[cap - 1] = 0;
    }
    if (rc != JOIN_OK) return rc;
    for (int i = 0; i < n; i++) new_bg[i] = p.new_bg[(size_t)i];
    *nkept = (int)p.kept.size();
    for (size_t i = 0; i < p.kept.size(); i++) {
        k_src[i] = p.kept[i].src_local;
        k_number[i] = p.kept[i].number;
        k_key[i] = p.kept[i].key;
        k_list[i] = p.kept[i].list;
        k_list_n[i] = p.kept[i].list_n;
        k_list_idx[i] = p.kept[i].list_idx;
    }
    *ninput = p.ninput;
    *nlists = p.nlists;
    *drops = p.drops ? 1 : 0;
    return rc;
}
uint64_t jp_drop(void) { return JOIN_DROP; }
}
