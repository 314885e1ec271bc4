// subseq_plan_host.cpp — lm_subseq_plan.h (the host's part of lm_index_subseqs) as a stand-alone program for
// tests/test_subseq_plan_cpu.py: commands on stdin, one answer line each, compared there with tests/subseq_model.py.
//   flanks <begin> <end> <rc> <up> <down>                       -> eStart eEnd
//   grid <interval> <nseqs> <size>*nseqs <ci>                   -> src,len,begin,end; for begin 1 .. s + 3, end begin .. s + 3, up and
//                                                                  down 0 .. s + 3, both strands (s = size of contig ci), in loop order
//   concat <rec_len> <eStart> <eEnd>                            -> status src len begin end
//   resolve <nrecs> (<nseqs> <id>*nseqs)*nrecs <seq_id | -> <seq_idx> -> rec seq_idx status
//   layout <n> <len>*n                                          -> goff ... total
//   pieces <budget> <n> <len>*n                                 -> g0:g1:r0:r1 ...
//   wrap <width> <seq | ->                                      -> the text, newlines as |
//   header <name> <begin> <end> <rc> <row with @ for tab | ->    -> the header line
//   extract <start> <len> <rc> <m> <hex of the region's bytes>  -> the groups of the region as ss_group writes them, zero bytes as .
//   status <n>                                                -> the text of a status
//   plan <interval> <up> <down> <ignore_errors> <nrecs> (<key> <genome id> <nseqs> (<id> <size>)*nseqs)*nrecs <nother> <key>*nother
//        <nregions> (<key | N> <genome id | -> <seq_id | -> <seq_idx> <rc> <begin> <end>)*nregions
//                                                               -> the whole plan of a call (ss_plan) over a table of records (in local
//                                                                  = chunk order; nother keys live on other shards): "ERR <refusal>" or
//                                                                  "OK" and status,local,key,seq_idx,rc,begin,end,src,len; per region
#include <cstdio>
#include <iostream>
#include <map>
#include <set>
#include <string>

#include "../lexicmap_amd/csrc/lm_subseq_plan.h"

namespace {
struct TableLookup : lm::SsLookup {
    std::vector<uint64_t> keys;
    std::vector<std::vector<std::string>> ids;
    std::vector<std::vector<int32_t>> sizes;
    std::vector<int64_t> lens;
    std::map<std::string, std::vector<int32_t>> by_name;
    std::set<uint64_t> other;
    int32_t local_of(uint64_t key) const override {
        for (size_t l = 0; l < keys.size(); l++)
            if (keys[l] == key) return (int32_t)l;
        return -1;
    }
    bool elsewhere(uint64_t key) const override { return other.count(key) != 0; }
    const std::vector<int32_t> *records_of(const char *genome_id) const override {
        const auto f = by_name.find(genome_id);
        return f == by_name.end() ? nullptr : &f->second;
    }
    lm::SsRecView record(int32_t local) const override {
        lm::SsRecView v;
        v.seq_sizes = sizes[(size_t)local].data();
        v.seq_ids = ids[(size_t)local].data();
        v.nseqs = (int32_t)ids[(size_t)local].size();
        v.len = lens[(size_t)local];
        v.key = keys[(size_t)local];
        return v;
    }
};
} // namespace

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "flanks") {
            long long b, e, up, down;
            int rc;
            std::cin >> b >> e >> rc >> up >> down;
            int64_t es, ee;
            lm::ss_flanks(b, e, rc != 0, up, down, &es, &ee);
            printf("%lld %lld\n", (long long)es, (long long)ee);
        } else if (cmd == "grid") {
            int interval, nseqs, ci;
            std::cin >> interval >> nseqs;
            std::vector<int32_t> sizes((size_t)nseqs);
            for (auto &x : sizes) std::cin >> x;
            std::cin >> ci;
            const int64_t top = sizes[(size_t)ci] + 3;
            for (int64_t b = 1; b <= top; b++)
                for (int64_t e = b; e <= top; e++)
                    for (int64_t up = 0; up <= top; up++)
                        for (int64_t down = 0; down <= top; down++)
                            for (int rc = 0; rc < 2; rc++) {
                                int64_t es, ee;
                                lm::ss_flanks(b, e, rc != 0, up, down, &es, &ee);
                                const lm::SsWindow w = lm::ss_contig_window(sizes.data(), ci, interval, es, ee);
                                if (w.status != lm::SS_OK) return 4;
                                printf("%lld,%lld,%lld,%lld;", (long long)w.src, (long long)w.len, (long long)w.begin, (long long)w.end);
                            }
            printf("\n");
        } else if (cmd == "concat") {
            long long len, es, ee;
            std::cin >> len >> es >> ee;
            const lm::SsWindow w = lm::ss_concat_window(len, es, ee);
            printf("%d %lld %lld %lld %lld\n", w.status, (long long)w.src, (long long)w.len, (long long)w.begin, (long long)w.end);
        } else if (cmd == "resolve") {
            int nrecs;
            std::cin >> nrecs;
            std::vector<std::vector<std::string>> ids((size_t)nrecs);
            std::vector<std::vector<int32_t>> sizes((size_t)nrecs);
            for (int r = 0; r < nrecs; r++) {
                int ns;
                std::cin >> ns;
                ids[(size_t)r].resize((size_t)ns);
                sizes[(size_t)r].assign((size_t)ns, 1);
                for (auto &x : ids[(size_t)r]) std::cin >> x;
            }
            std::string seq_id;
            int seq_idx;
            std::cin >> seq_id >> seq_idx;
            std::vector<lm::SsRecView> recs((size_t)nrecs);
            for (int r = 0; r < nrecs; r++) {
                recs[(size_t)r].seq_sizes = sizes[(size_t)r].data();
                recs[(size_t)r].seq_ids = ids[(size_t)r].data();
                recs[(size_t)r].nseqs = (int32_t)ids[(size_t)r].size();
            }
            const lm::SsResolved x = lm::ss_resolve(recs.data(), nrecs, seq_id == "-" ? nullptr : seq_id.c_str(), seq_idx);
            printf("%d %d %d\n", x.rec, x.seq_idx, x.status);
        } else if (cmd == "layout" || cmd == "pieces") {
            long long budget = 0;
            size_t n;
            if (cmd == "pieces") std::cin >> budget;
            std::cin >> n;
            std::vector<int64_t> len(n), goff(n + 1);
            for (auto &x : len) std::cin >> x;
            lm::ss_layout(len.data(), n, goff.data());
            if (cmd == "layout") {
                for (int64_t g : goff) printf("%lld ", (long long)g);
            } else {
                std::vector<lm::SsPiece> out;
                lm::ss_pieces(goff.data(), n, budget, out);
                for (const auto &p : out) printf("%lld:%lld:%lld:%lld ", (long long)p.g0, (long long)p.g1, (long long)p.r0, (long long)p.r1);
            }
            printf("\n");
        } else if (cmd == "wrap") {
            int width;
            std::string s, out;
            std::cin >> width >> s;
            if (s == "-") s.clear();
            lm::ss_wrap(out, s.data(), (int64_t)s.size(), width);
            for (char &c : out)
                if (c == '\n') c = '|';
            printf("%s\n", out.c_str());
        } else if (cmd == "header") {
            std::string name, row, out;
            long long b, e;
            int rc;
            std::cin >> name >> b >> e >> rc >> row;
            for (char &c : row)
                if (c == '@') c = '\t';
            lm::ss_header(out, name.c_str(), b, e, rc != 0, row == "-" ? nullptr : row.c_str());
            printf("%s\n", out.c_str());
        } else if (cmd == "extract") {
            // the lanes of k_subseq_extract over one region; the allocation ends with the region's last byte and begins m bytes
            // before its first one, so that AddressSanitizer sees any load outside (m = 0: on both sides)
            long long start, len;
            int rc, m;
            std::string hex;
            std::cin >> start >> len >> rc >> m >> hex;
            const int64_t lo = start >> 2, hi = (start + len - 1) >> 2, nbytes = hi - lo + 1;
            if ((int64_t)hex.size() != 2 * nbytes) return 5;
            uint8_t *buf = new uint8_t[(size_t)(nbytes + m)];
            for (int i = 0; i < m; i++) buf[i] = 0xff;
            for (int64_t i = 0; i < nbytes; i++) buf[m + i] = (uint8_t)std::stoi(hex.substr((size_t)(2 * i), 2), nullptr, 16);
            const uint8_t *src = buf + m - lo;
            std::string out;
            for (int64_t o0 = 0; o0 < len; o0 += LM_SS_GROUP) {
                uint32_t w[4];
                lm::ss_group(src, start, len, rc != 0, o0, w);
                for (int j = 0; j < LM_SS_GROUP; j++) {
                    const char c = (char)((w[j >> 2] >> (8 * (j & 3))) & 0xff);
                    out.push_back(c ? c : '.');
                }
            }
            delete[] buf;
            printf("%s\n", out.c_str());
        } else if (cmd == "status") {
            int st;
            std::cin >> st;
            printf("%s\n", lm::ss_status_text(st));
        } else if (cmd == "plan") {
            int interval, ignore;
            long long up, down;
            size_t nrecs, nother, nreg;
            std::cin >> interval >> up >> down >> ignore >> nrecs;
            TableLookup L;
            for (size_t l = 0; l < nrecs; l++) {
                unsigned long long key;
                std::string gid;
                size_t ns;
                std::cin >> key >> gid >> ns;
                L.keys.push_back(key);
                L.by_name[gid].push_back((int32_t)l);
                L.ids.emplace_back(ns);
                L.sizes.emplace_back(ns);
                int64_t len = ns ? (int64_t)interval * (int64_t)(ns - 1) : 0;
                for (size_t c = 0; c < ns; c++) {
                    std::cin >> L.ids.back()[c] >> L.sizes.back()[c];
                    len += L.sizes.back()[c];
                }
                L.lens.push_back(len);
            }
            std::cin >> nother;
            for (size_t i = 0; i < nother; i++) {
                unsigned long long key;
                std::cin >> key;
                L.other.insert(key);
            }
            std::cin >> nreg;
            std::vector<std::string> gids(nreg), sids(nreg);
            std::vector<lm::SsRegion> regions(nreg);
            for (size_t i = 0; i < nreg; i++) {
                std::string key;
                long long b, e;
                std::cin >> key >> gids[i] >> sids[i] >> regions[i].seq_idx >> regions[i].rc >> b >> e;
                regions[i].key = key == "N" ? LM_SS_BY_NAME : std::stoull(key);
                regions[i].genome_id = gids[i] == "-" ? nullptr : gids[i].c_str();
                regions[i].seq_id = sids[i] == "-" ? nullptr : sids[i].c_str();
                regions[i].begin = b;
                regions[i].end = e;
            }
            std::vector<lm::SsItem> items;
            std::string err;
            const bool ok = lm::ss_plan(L, interval, "plan", nreg, [&](size_t i) { return regions[i]; }, up, down, ignore != 0, items, err,
                                        [](int64_t m, auto f) { f((int64_t)0, m); });
            if (!ok) {
                printf("ERR %s\n", err.c_str());
            } else {
                printf("OK ");
                for (const lm::SsItem &it : items)
                    printf("%d,%d,%llu,%d,%d,%lld,%lld,%lld,%lld;", it.status, it.local, (unsigned long long)it.key, it.seq_idx, it.rc, (long long)it.w.begin,
                           (long long)it.w.end, (long long)it.w.src, (long long)it.w.len);
                printf("\n");
            }
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
