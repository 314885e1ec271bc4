// Stand-alone form of tests/pa_rule_map_host.cpp for the sanitizers: pa_rule_map_main <sets file> builds the filter of every
// k-mer set of the file and runs the exhaustive check of the rule map and the no-growth check on it.
// The file (host byte order): int32 number of sets, then per set int32 n, int32 log, n x uint64 k-mers (K = 31).
// Prints one line per set; exit status 1 on the first failure.  Test infrastructure only (tests/test_pa_rule_map_cpu.py).
#include "pa_rule_map_host.cpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t nsets = 0;
    if (fread(&nsets, sizeof nsets, 1, f) != 1) return 2;
    const int K = 31;
    for (int s = 0; s < nsets; s++) {
        int32_t hdr[2];
        if (fread(hdr, sizeof hdr, 1, f) != 1) return 2;
        const int n = hdr[0], log = hdr[1];
        std::vector<uint64_t> keys((size_t)n);
        if (n > 0 && fread(keys.data(), sizeof(uint64_t), (size_t)n, f) != (size_t)n) return 2;
        std::vector<uint32_t> bits((size_t)rm_bits_words(log), 0u);
        rm_build(keys.data(), n, K, log, bits.data());
        const long long nset = rm_check_exhaustive(keys.data(), n, K, bits.data(), log);
        if (nset < 0) {
            printf("set %d: rule map differs from the literal rule at p9 = %lld\n", s, -1 - nset);
            return 1;
        }
        for (int p = 11; p <= 15; p += 2) {
            long long out[2];
            const long long bad = rm_no_growth(keys.data(), n, K, bits.data(), log, p, 1000u + (unsigned)s, 200000, out);
            if (bad) {
                printf("set %d, p %d: %lld keys pass lm_pa_candidate3 and not lm_pa_candidate2\n", s, p, bad);
                return 1;
            }
        }
        printf("set %d: n %d log %d, %lld bits of the rule map set\n", s, n, log, nset);
    }
    fclose(f);
    return 0;
}
