// Host build of the seed-distance rule of k_sd_pass (lexicmap_amd/csrc/lm_seed_dist.h) for tests/test_seed_dist_cpu.py: a
// stand-alone program (built with -fsanitize=address,undefined) that walks hand-made position lists entry by entry, as the
// kernel's lanes do - each entry from its own position and the one before only - and compares with a plain sequential loop
// over the contigs.  Prints one line per case, exits 1 on the first difference.
#include "../lexicmap_amd/csrc/lm_seed_dist.h"

#include <cstdio>
#include <vector>

using namespace lm;

struct Row {
    int32_t contig;
    uint32_t pos, pos_in_contig, dist;
    bool operator==(const Row &o) const { return contig == o.contig && pos == o.pos && pos_in_contig == o.pos_in_contig && dist == o.dist; }
};

// the plain loop: contig by contig, the positions that fall into [s_c, s_{c+1}) in order
static std::vector<Row> plain(const std::vector<int32_t> &len, int interval, const std::vector<uint32_t> &pos, uint32_t min_dist, int *seedless) {
    std::vector<Row> out;
    size_t i = 0;
    uint32_t s = 0;
    *seedless = 0;
    for (size_t c = 0; c < len.size(); c++) {
        const bool last = c + 1 == len.size();
        const uint32_t next = s + (uint32_t)len[c] + (uint32_t)interval;
        uint32_t pre = s;
        bool any = false;
        while (i < pos.size() && (last || pos[i] < next)) {
            const uint32_t d = pos[i] - pre;
            if (d >= min_dist) out.push_back(Row{(int32_t)c, pos[i], pos[i] - s, d});
            pre = pos[i];
            any = true;
            i++;
        }
        if (!any) (*seedless)++;
        s = next;
    }
    return out;
}

static std::vector<Row> by_entry(const std::vector<int32_t> &len, int interval, const std::vector<uint32_t> &pos, uint32_t min_dist, int *seedless) {
    std::vector<uint32_t> starts(len.size());
    sd_contig_starts(len.data(), (int32_t)len.size(), interval, starts.data());
    std::vector<Row> out;
    int seeded = 0;
    for (size_t e = 0; e < pos.size(); e++) {
        const SdEntry en = sd_entry(starts.data(), (int32_t)starts.size(), pos[e], e > 0, e > 0 ? pos[e - 1] : 0u);
        if (en.first) seeded++;
        if (sd_reported(en.dist, min_dist)) out.push_back(Row{en.contig, pos[e], pos[e] - en.start, en.dist});
    }
    *seedless = (int)len.size() - seeded;
    return out;
}

static int check(const char *name, const std::vector<int32_t> &len, int interval, const std::vector<uint32_t> &pos, int want_rows0, int want_seedless) {
    for (uint32_t min_dist : {0u, 1u, 50u, 200u, 100000u}) {
        int sa = 0, sb = 0;
        const std::vector<Row> a = plain(len, interval, pos, min_dist, &sa), b = by_entry(len, interval, pos, min_dist, &sb);
        if (!(a == b) || sa != sb || sa != want_seedless || (min_dist == 0 && (int)a.size() != want_rows0)) {
            printf("FAIL %s min_dist %u: %zu / %zu rows, %d / %d / %d seedless contigs\n", name, min_dist, a.size(), b.size(), sa, sb, want_seedless);
            return 1;
        }
    }
    printf("ok %s\n", name);
    return 0;
}

int main() {
    int bad = 0;
    const int K = 31;
    // contigs of 5000, 40, 3000 bases, interval 1000: starts 0, 6000, 7040
    const std::vector<int32_t> three = {5000, 40, 3000};
    std::vector<uint32_t> starts(3);
    sd_contig_starts(three.data(), 3, 1000, starts.data());
    if (starts[0] != 0 || starts[1] != 6000 || starts[2] != 7040) {
        printf("FAIL contig starts %u %u %u\n", starts[0], starts[1], starts[2]);
        return 1;
    }
    // the contig search at every boundary
    const uint32_t probe[] = {0, 1, 4999, 5000, 5999, 6000, 6039, 7039, 7040, 10039, 0x0fffffff};
    for (uint32_t p : probe) {
        int32_t c = 0;
        for (int32_t x = 0; x < 3; x++)
            if (starts[(size_t)x] <= p) c = x;
        if (sd_contig(starts.data(), 3, p) != c) {
            printf("FAIL contig of %u\n", p);
            return 1;
        }
    }
    // a position exactly at s_c (dist 0 as the first of its contig) and the last k-mer of a contig
    bad |= check("position at a contig start, last k-mer of a contig", three, 1000, {0, 120, (uint32_t)(5000 - K), 6000, 6009, 7040, 7040 + 3000 - K}, 7, 0);
    // a contig without seeds between two seeded ones
    bad |= check("seedless contig in the middle", three, 1000, {10, 300, 4000, 7100, 7300, 9000}, 6, 1);
    // duplicates: inside a contig, at a contig's first position, three times
    bad |= check("duplicates", three, 1000, {10, 10, 500, 6003, 6003, 8000, 8000, 8000}, 8, 0);
    // a single-contig record
    bad |= check("single contig", {120000}, 1000, {0, 3, 99, 40000, 119969}, 5, 0);
    // an empty list
    bad |= check("empty list", three, 1000, {}, 0, 3);
    // only the last contig is seeded; interval 0
    bad |= check("only the last contig", three, 1000, {7041, 7090}, 2, 2);
    bad |= check("interval 0", {100, 100, 100}, 0, {0, 99, 100, 199, 200, 260}, 6, 0);
    // the histogram counter
    if (sd_bin(0, 16, 25) != 0 || sd_bin(24, 16, 25) != 0 || sd_bin(25, 16, 25) != 1 || sd_bin(374, 16, 25) != 14 || sd_bin(375, 16, 25) != 15 ||
        sd_bin(1000000, 16, 25) != 15 || sd_bin(7, 1, 1) != 0) {
        printf("FAIL histogram counter\n");
        bad = 1;
    }
    return bad;
}
