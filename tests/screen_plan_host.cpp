// screen_plan_host.cpp — lm_screen_plan.h (the host's part of lm_index_screen_genomes) as a stand-alone program for
// tests/test_screen_plan_cpu.py: commands on stdin, one answer line each, compared there with tests/screen_model.py.
//   windows <len> <windows>                      -> start:len ...
//   layout <k> <n> <len>*n                       -> total start... | s:e ...
//   pieces <soft> <hard> <M> <count>*M           -> m0:m1:tuples ...   or   bad <mask>
//   partials <n> (<query> <local> <score> <score2> <hit_kmers> <hit_masks>)*n -> query:local:score:score2:hit_kmers:hit_masks:<entries> ...
//   rows <top_n> <n> (<query> <key> <list> <score>)*n -> query:score:detail_key:key,key.. ...
#include <cstdio>
#include <iostream>
#include <string>

#include "../lexicmap_amd/csrc/lm_screen_plan.h"

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "windows") {
            long long len;
            int w;
            std::cin >> len >> w;
            std::vector<lm::ScreenWindow> out;
            lm::screen_windows(len, w, out);
            for (const auto &x : out) printf("%lld:%lld ", (long long)x.start, (long long)x.len);
            printf("\n");
        } else if (cmd == "layout") {
            int k;
            size_t n;
            std::cin >> k >> n;
            std::vector<uint32_t> cl(n);
            for (auto &x : cl) std::cin >> x;
            lm::ScreenLayout L;
            lm::screen_layout(cl.data(), n, k, L);
            printf("%lld", (long long)L.len);
            for (auto s : L.start) printf(" %lld", (long long)s);
            printf(" |");
            for (size_t i = 0; i < L.reg_s.size(); i++) printf(" %d:%d", L.reg_s[i], L.reg_e[i]);
            printf("\n");
        } else if (cmd == "pieces") {
            long long soft, hard;
            int M;
            std::cin >> soft >> hard >> M;
            std::vector<uint64_t> c((size_t)M);
            for (auto &x : c) std::cin >> x;
            std::vector<lm::ScreenPiece> out;
            int bad = -1;
            if (!lm::screen_pieces(c.data(), M, soft, hard, out, &bad)) {
                printf("bad %d\n", bad);
                continue;
            }
            for (const auto &p : out) printf("%d:%d:%lld ", p.m0, p.m1, (long long)p.tuples);
            printf("\n");
        } else if (cmd == "partials") {
            size_t n;
            std::cin >> n;
            std::vector<lm::ScreenPartial> in(n), out;
            for (auto &p : in) {
                std::cin >> p.query >> p.local >> p.score >> p.score2 >> p.hit_kmers >> p.hit_masks;
                p.pref_off = 0;
            }
            std::vector<std::vector<size_t>> chain;
            lm::screen_merge_partials(in, out, chain);
            for (size_t i = 0; i < out.size(); i++) {
                printf("%u:%lld:%llu:%llu:%llu:%u:", out[i].query, (long long)out[i].local, (unsigned long long)out[i].score,
                       (unsigned long long)out[i].score2, (unsigned long long)out[i].hit_kmers, out[i].hit_masks);
                for (size_t j = 0; j < chain[i].size(); j++) printf("%s%zu", j ? "," : "", chain[i][j]);
                printf(" ");
            }
            printf("\n");
        } else if (cmd == "rows") {
            int top_n;
            size_t n;
            std::cin >> top_n >> n;
            std::vector<lm::ScreenHit> hits(n);
            for (auto &h : hits) std::cin >> h.query >> h.key >> h.list >> h.score;
            std::vector<lm::ScreenRow> rows;
            lm::screen_rows(hits, top_n, rows);
            for (const auto &r : rows) {
                printf("%u:%llu:%llu:", r.query, (unsigned long long)r.score, (unsigned long long)hits[r.detail].key);
                for (size_t j = 0; j < r.keys.size(); j++) printf("%s%llu", j ? "," : "", (unsigned long long)r.keys[j]);
                printf(" ");
            }
            printf("\n");
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
