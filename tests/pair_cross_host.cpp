// pair_cross_host.cpp — lm_pair_cross_plan.h (the host's part of the pairs across shards) as a stand-alone program for
// tests/test_pair_cross_plan_cpu.py: commands on stdin, one answer line each.
//   blob <k> <M> <masks> <ns> <fp> <nrec> (<key> <idlen> <idchar>)*nrec <offset>*(ns + 1) <nent> (<kmer> <rec>)*nent
//        writes the blob (the id of a record is <idchar> repeated <idlen> times), parses it back and prints
//        ok <bytes> <hex of the blob> | <k> <M> <masks> <ns> <fp> <nrec> <nent> | key:idlen:first+last id char ... | offsets | kmer:rec ...
//        (the hex only when the blob is at most 4096 bytes, else "-")
//   parse <hex>                                   -> ok <nrec> <nent>   or   refused <text>
//   parsecopy <hex>                               the same on a copy that ends at the end of its heap block and starts at an odd address
//   fits <hex> <k> <M> <fp> <masks> <ns>          -> ok   or   refused <text>
//   union <nown> <key>*nown <nblobs> (<n> <key>*n)*nblobs -> key:src:idx ... | own slots | blob slots ;...   or   refused <text>
//   merge <np> (<n> (<key1> <key2> <n_masks> <sum>)*n)*np -> part:row ...   or   refused <text>
//   fingerprint <M> <mask>*M                      -> the fingerprint
#include <cstdio>
#include <iostream>
#include <string>

#include "../lexicmap_amd/csrc/lm_pair_cross_plan.h"

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    auto v = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)(v(s[i]) * 16 + v(s[i + 1])));
    return out;
}
static std::string oneline(std::string s) {
    for (char &c : s)
        if (c == '\n') c = ' ';
    return s;
}
struct Row {
    uint64_t key1, key2;
    uint32_t n_masks, sum_prefix;
};

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        std::string err;
        if (cmd == "blob") {
            lm::PairBlobHead hd;
            std::cin >> hd.k >> hd.M >> hd.masks >> hd.total_masks >> hd.fingerprint >> hd.records;
            std::vector<uint64_t> keys((size_t)hd.records);
            std::vector<std::string> ids((size_t)hd.records);
            for (int64_t r = 0; r < hd.records; r++) {
                size_t len;
                char c;
                std::cin >> keys[(size_t)r] >> len >> c;
                ids[(size_t)r] = std::string(len, c);
                hd.id_bytes += (int64_t)len;
            }
            std::vector<int64_t> off((size_t)hd.total_masks + 1);
            for (auto &x : off) std::cin >> x;
            std::cin >> hd.entries;
            std::vector<uint64_t> kmers((size_t)hd.entries);
            std::vector<uint32_t> recs((size_t)hd.entries);
            for (int64_t e = 0; e < hd.entries; e++) std::cin >> kmers[(size_t)e] >> recs[(size_t)e];
            const size_t nb = lm::pair_blob_size(hd.total_masks, hd.records, hd.entries, hd.id_bytes);
            std::vector<uint8_t> blob(nb);
            if (!lm::pair_blob_write(hd, keys.data(), ids, off.data(), kmers.data(), recs.data(), blob.data(), err)) {
                printf("refused %s\n", oneline(err).c_str());
                continue;
            }
            lm::PairBlobView v;
            if (!lm::pair_blob_parse(blob.data(), blob.size(), v, err)) {
                printf("refused %s\n", oneline(err).c_str());
                continue;
            }
            printf("ok %zu ", nb);
            if (nb <= 4096)
                for (uint8_t b : blob) printf("%02x", b);
            else printf("-");
            printf(" | %d %d %d %d %llu %lld %lld |", v.hd.k, v.hd.M, v.hd.masks, v.hd.total_masks, (unsigned long long)v.hd.fingerprint,
                   (long long)v.hd.records, (long long)v.hd.entries);
            int64_t at = 0;
            for (int64_t r = 0; r < v.hd.records; r++) {
                const int l = v.idlen(r);
                printf(" %llu:%d:", (unsigned long long)v.key(r), l);
                if (l) printf("%c%c", (char)v.ids[at], (char)v.ids[at + l - 1]);
                at += l;
            }
            printf(" |");
            for (int32_t s = 0; s <= v.hd.total_masks; s++) printf(" %lld", (long long)v.offset(s));
            printf(" |");
            for (int64_t e = 0; e < v.hd.entries; e++) printf(" %llu:%u", (unsigned long long)v.kmer(e), v.rec(e));
            printf("\n");
        } else if (cmd == "parse" || cmd == "parsecopy") {
            std::string hex;
            std::cin >> hex;
            const std::vector<uint8_t> raw = unhex(hex);
            lm::PairBlobView v;
            bool ok;
            if (cmd == "parse") {
                ok = lm::pair_blob_parse(raw.data(), raw.size(), v, err);
            } else { // an exact heap block behind one spare byte: a read past the end or an aligned load is a sanitizer report
                uint8_t *blk = new uint8_t[raw.size() + 1];
                if (!raw.empty()) memcpy(blk + 1, raw.data(), raw.size());
                ok = lm::pair_blob_parse(blk + 1, raw.size(), v, err);
                if (ok) { // every section is readable to its end
                    uint64_t sum = 0;
                    for (int64_t r = 0; r < v.hd.records; r++) sum += v.key(r) + v.idlen(r);
                    for (int64_t i = 0; i < v.hd.id_bytes; i++) sum += v.ids[i];
                    for (int64_t e = 0; e < v.hd.entries; e++) sum += v.kmer(e) + v.rec(e);
                    if (sum == 0x123456789abcdefull) printf(" ");
                }
                delete[] blk;
            }
            if (ok) printf("ok %lld %lld\n", (long long)v.hd.records, (long long)v.hd.entries);
            else if (err.empty()) return 4; // refused without a text
            else printf("refused %s\n", oneline(err).c_str());
        } else if (cmd == "fits") {
            std::string hex;
            int k, M;
            uint64_t fp;
            int32_t masks, ns;
            std::cin >> hex >> k >> M >> fp >> masks >> ns;
            const std::vector<uint8_t> raw = unhex(hex);
            lm::PairBlobView v;
            if (!lm::pair_blob_parse(raw.data(), raw.size(), v, err)) return 5;
            if (lm::pair_blob_fits(v.hd, k, M, fp, masks, ns, err)) printf("ok\n");
            else printf("refused %s\n", oneline(err).c_str());
        } else if (cmd == "union") {
            size_t nown, nblobs;
            std::cin >> nown;
            std::vector<uint64_t> own(nown);
            for (auto &x : own) std::cin >> x;
            std::cin >> nblobs;
            std::vector<std::vector<uint64_t>> blobs(nblobs);
            for (auto &b : blobs) {
                size_t n;
                std::cin >> n;
                b.resize(n);
                for (auto &x : b) std::cin >> x;
            }
            lm::PairSlots s;
            if (!lm::pair_slot_union(own, blobs, s, err)) {
                printf("refused %s\n", oneline(err).c_str());
                continue;
            }
            for (size_t i = 0; i < s.key.size(); i++) printf("%llu:%d:%lld ", (unsigned long long)s.key[i], s.src[i], (long long)s.idx[i]);
            printf("|");
            for (uint32_t x : s.own_slot) printf(" %u", x);
            printf(" |");
            for (const auto &b : s.blob_slot) {
                for (uint32_t x : b) printf(" %u", x);
                printf(" ;");
            }
            printf("\n");
        } else if (cmd == "merge") {
            size_t np;
            std::cin >> np;
            std::vector<std::vector<Row>> parts(np);
            for (auto &p : parts) {
                size_t n;
                std::cin >> n;
                p.resize(n);
                for (auto &r : p) std::cin >> r.key1 >> r.key2 >> r.n_masks >> r.sum_prefix;
            }
            std::vector<const Row *> rp;
            std::vector<size_t> rn;
            for (const auto &p : parts) {
                rp.push_back(p.data());
                rn.push_back(p.size());
            }
            std::vector<std::pair<uint32_t, size_t>> order;
            if (!lm::pair_merge_plan(rp.data(), rn.data(), np, order, err)) {
                printf("refused %s\n", oneline(err).c_str());
                continue;
            }
            for (const auto &o : order) printf("%u:%zu ", o.first, o.second);
            printf("\n");
        } else if (cmd == "fingerprint") {
            size_t M;
            std::cin >> M;
            std::vector<uint64_t> masks(M);
            for (auto &x : masks) std::cin >> x;
            printf("%llu\n", (unsigned long long)lm::pair_mask_fingerprint(masks.data(), (int64_t)M));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
