// pair_plan_host.cpp — lm_pair_plan.h (the host's part of lm_index_genome_pairs) as a stand-alone program for
// tests/test_pair_plan_cpu.py: commands on stdin, one answer line each, compared there with tests/pair_model.py.
//   select <k> <nmasks> <M> <mask>*M                         -> total mask ...   or   refused
//   required <fraction> <total>                              -> required
//   pieces <soft> <hard> <slot_bits> <ns> <count>*ns          -> s0:s1:tuples:mask_bits ...   or   bad <selected mask | -1>
//   add <masks_left> <required> <nt> (<pair> <n> <sum>)*nt <np> (<pair> <n> <sum>)*np -> pair:n:sum ...
//   order <n> (<pair> <n_masks> <sum>)*n                      -> pair:n:sum ...
//   format <cap> <min_prefix> <total> <n_masks> <sum> <g1> <g2> -> <length>|<text>
//   header                                                    -> the header line
#include <cstdio>
#include <iostream>
#include <string>

#include "../lexicmap_amd/csrc/lm_pair_plan.h"

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "select") {
            int k, M;
            long long nmasks;
            std::cin >> k >> nmasks >> M;
            std::vector<uint64_t> masks((size_t)M);
            for (auto &x : masks) std::cin >> x;
            std::vector<int32_t> sel;
            std::string err;
            if (!lm::pair_select_masks(masks.data(), M, k, nmasks, sel, err)) {
                printf("refused\n");
                continue;
            }
            printf("%zu", sel.size());
            for (int32_t m : sel) printf(" %d", m);
            printf("\n");
        } else if (cmd == "required") {
            double f;
            long long total;
            std::cin >> f >> total;
            printf("%lld\n", (long long)lm::pair_required(f, total));
        } else if (cmd == "pieces") {
            long long soft, hard;
            int sb, ns;
            std::cin >> soft >> hard >> sb >> ns;
            std::vector<int64_t> c((size_t)ns);
            for (auto &x : c) std::cin >> x;
            std::vector<lm::PairPiece> out;
            int32_t bad = -2;
            if (!lm::pair_pieces(c.data(), ns, soft, hard, sb, out, &bad)) {
                printf("bad %d\n", bad);
                continue;
            }
            for (const auto &p : out) printf("%d:%d:%lld:%d ", p.s0, p.s1, (long long)p.tuples, p.mask_bits);
            printf("\n");
        } else if (cmd == "add") {
            long long left, req;
            size_t nt, np;
            std::cin >> left >> req >> nt;
            std::vector<lm::PairRow> tab(nt), out;
            for (auto &r : tab) std::cin >> r.pair >> r.n_masks >> r.sum_prefix;
            std::cin >> np;
            std::vector<lm::PairRow> part(np);
            for (auto &r : part) std::cin >> r.pair >> r.n_masks >> r.sum_prefix;
            lm::pair_add_partials(tab, part, left, req, out);
            for (const auto &r : out) printf("%llu:%u:%u ", (unsigned long long)r.pair, r.n_masks, r.sum_prefix);
            printf("\n");
        } else if (cmd == "order") {
            size_t n;
            std::cin >> n;
            std::vector<lm::PairRow> rows(n);
            for (auto &r : rows) std::cin >> r.pair >> r.n_masks >> r.sum_prefix;
            lm::pair_order(rows);
            for (const auto &r : rows) printf("%llu:%u:%u ", (unsigned long long)r.pair, r.n_masks, r.sum_prefix);
            printf("\n");
        } else if (cmd == "format") {
            size_t cap;
            int p, total;
            uint32_t n, sum;
            std::string g1, g2;
            std::cin >> cap >> p >> total >> n >> sum >> g1 >> g2;
            std::vector<char> buf(cap + 1, '#');
            const int len = lm::pair_format_row(g1.c_str(), g2.c_str(), p, n, sum, total, cap ? buf.data() : nullptr, cap);
            if (buf[cap] != '#') return 3; // wrote past the capacity
            printf("%d|%s\n", len, cap ? buf.data() : "");
        } else if (cmd == "header") {
            printf("%s\n", lm::pair_header());
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
