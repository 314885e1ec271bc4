// Host build of the mask-set rule of the index builder (lexicmap_amd/csrc/lm_mask_plan.h) for tests/test_mask_plan_cpu.py: a
// stand-alone program (built with -fsanitize=address,undefined) that reads cases from the file named on its command line and
// prints what plan_masks makes of each; the test computes the expectations in Python.
//   in:   "case <name> <k> <n>" followed by n masks in hex         out: "<name> ok <p> <max per prefix> <once or twice> <pfx_first ...>"
//                                                                       "<name> refused <text>"
//         "prefix <n>"                                                  "prefix <n> <p>"
#include "../lexicmap_amd/csrc/lm_mask_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char word[64], name[64];
    while (fscanf(f, "%63s", word) == 1) {
        if (!strcmp(word, "prefix")) {
            unsigned long long n = 0;
            if (fscanf(f, "%llu", &n) != 1) return 2;
            printf("prefix %llu %d\n", n, lm::mask_plan_prefix((size_t)n));
            continue;
        }
        int k = 0;
        unsigned long long n = 0;
        if (strcmp(word, "case") || fscanf(f, "%63s %d %llu", name, &k, &n) != 3) return 2;
        std::vector<uint64_t> masks((size_t)n); // exactly n: a read past the set is the sanitizer's to find
        for (auto &m : masks)
            if (fscanf(f, "%" SCNx64, &m) != 1) return 2;
        lm::MaskPlan mp;
        std::string err;
        if (!lm::plan_masks(k, masks.data(), masks.size(), mp, err)) {
            printf("%s refused %s\n", name, err.c_str());
            continue;
        }
        printf("%s ok %d %d %d", name, mp.p, mp.max_per_prefix, mp.once_or_twice ? 1 : 0);
        for (int32_t v : mp.pfx_first) printf(" %d", v);
        printf("\n");
    }
    fclose(f);
    return 0;
}
