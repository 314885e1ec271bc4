// lm_join_plan.h — the record planner of lm_index_builder_add_index (lm_builder.hip): which genome records of a resident
// index are appended to a builder, under which new keys and chunk-list numbers, and what is refused.  Host-only and free of
// HIP, so that it is tested without a device (tests/join_plan_host.cpp).  The device reads one thing of it: new_bg, the key
// rewrite table of k_sp_dump_range (lm_seedpack.hip).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "lm_build_plan.h"

namespace lm {

// new_bg of a record that is not kept: no seed of it reaches the packer
static const uint64_t JOIN_DROP = ~(uint64_t)0;

// One record of the source, in the source's record order.  list < 0: the genome is not split; otherwise the number of its
// chunk list in the source (HostIndex::chunk_of), the length of that list and the record's place in it.
struct JoinSrcRecord {
    uint64_t key = 0; // batch << 17 | index, as the source's seed values carry it
    int list = -1, list_n = 0, list_idx = 0;
};

struct JoinKept {
    int64_t src_local = 0; // the record's place in the source's table
    int64_t number = 0;    // its record number in the builder
    uint64_t key = 0;      // build_genome_key(number, batch_size)
    int list = -1, list_n = 0, list_idx = 0; // chunk list in the builder (list ids moved up), -1: none
};

enum { JOIN_OK = 0, JOIN_EMPTY = 1, JOIN_UNKNOWN_KEY = 2, JOIN_REPEATED_KEY = 3, JOIN_HALF_SPLIT = 4, JOIN_TOO_MANY = 5 };

struct JoinPlan {
    std::vector<uint64_t> new_bg; // [source records] new key or JOIN_DROP
    std::vector<JoinKept> kept;   // in the source's order
    int64_t ninput = 0;           // input genomes among them: a split genome counts once
    int nlists = 0;               // the builder's next list id afterwards
    bool drops = false;           // some record is not kept: the decode kernel compacts
};

// keep == nullptr: every record.  Otherwise keep[0 .. nkeep) are keys of the source; the kept records still come in the
// source's order.  next_record / next_list: the builder's record count and next chunk-list id; a kept chunk list gets
// next_list + its rank among the kept lists by first record, which is the id one build of the same genomes in the same
// order gives it.  JOIN_OK, or the reason with a text in `err` (nothing of `out` is to be used then).
static inline int plan_join(const std::vector<JoinSrcRecord> &src, const uint64_t *keep, size_t nkeep, int64_t next_record, int batch_size,
                            int next_list, JoinPlan &out, std::string &err) {
    out = JoinPlan();
    const size_t n = src.size();
    std::vector<uint8_t> sel(n, keep ? 0 : 1);
    if (keep) {
        if (nkeep == 0) {
            err = "the keep list is empty: no record is selected";
            return JOIN_EMPTY;
        }
        std::unordered_map<uint64_t, size_t> at;
        for (size_t l = 0; l < n; l++) at[src[l].key] = l;
        for (size_t i = 0; i < nkeep; i++) {
            const auto it = at.find(keep[i]);
            if (it == at.end()) {
                err = "the keep list names the key " + std::to_string(keep[i]) + " (batch " + std::to_string(keep[i] >> 17) + ", index " +
                      std::to_string(keep[i] & 0x1ffff) + "), which is no record of the source index";
                return JOIN_UNKNOWN_KEY;
            }
            if (sel[it->second]) {
                err = "the keep list names the key " + std::to_string(keep[i]) + " twice";
                return JOIN_REPEATED_KEY;
            }
            sel[it->second] = 1;
        }
    } else if (n == 0) {
        err = "the source index holds no record";
        return JOIN_EMPTY;
    }
    // a split genome: all of its records or none
    std::unordered_map<int, std::pair<int, int>> lists; // source list -> (records in the table, records kept)
    for (size_t l = 0; l < n; l++)
        if (src[l].list >= 0) {
            auto &c = lists[src[l].list];
            c.first++;
            c.second += sel[l];
        }
    for (size_t l = 0; l < n; l++)
        if (src[l].list >= 0 && sel[l]) {
            const auto &c = lists[src[l].list];
            if (c.second != c.first || c.first != src[l].list_n) {
                err = "the keep list names " + std::to_string(c.second) + " of the " + std::to_string(std::max(c.first, src[l].list_n)) +
                      " records of a split genome (key " + std::to_string(src[l].key) + " is one of them): all of its records or none";
                return JOIN_HALF_SPLIT;
            }
        }
    std::unordered_map<int, int> new_list;
    out.new_bg.assign(n, JOIN_DROP);
    out.nlists = next_list;
    int64_t number = next_record;
    for (size_t l = 0; l < n; l++) {
        if (!sel[l]) {
            out.drops = true;
            continue;
        }
        if (number / batch_size >= ((int64_t)1 << 30)) {
            err = "more genome records than keys";
            return JOIN_TOO_MANY;
        }
        JoinKept k;
        k.src_local = (int64_t)l;
        k.number = number;
        k.key = build_genome_key(number, batch_size);
        if (src[l].list >= 0) {
            auto it = new_list.find(src[l].list);
            if (it == new_list.end()) {
                it = new_list.emplace(src[l].list, out.nlists++).first;
                out.ninput++;
            }
            k.list = it->second;
            k.list_n = src[l].list_n;
            k.list_idx = src[l].list_idx;
        } else {
            out.ninput++;
        }
        out.new_bg[l] = k.key;
        out.kept.push_back(k);
        number++;
    }
    return JOIN_OK;
}

} // namespace lm
