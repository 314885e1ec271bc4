"""Windows that reach every branch of the rule map of the pseudo-alignment filter (lm_pa_candidate3, lm_algos.h), added to the
fixture of tests/pa_cases.py.  TEST INFRASTRUCTURE ONLY.

One short query and the same query followed by 16 500 unrelated bases (its filter then has a global 11-base bitmap: Bloom hits of
the LDS filter wait in the pending list), against windows of 3 000, 10 000 and 50 000 bases (p = 11, 13, 15) in both
orientations.  Every window holds, as a k-mer and as the reverse complement of one (so that either strand of the search meets
it), keys of the branches

  all7      bases [7, p) all A, no query k-mer with the key's 11-base prefix (query k-mers share exactly 7 and 8 bases);
  base8_A   base 8 an A, base 7 not, query k-mers with the key's 9-base prefix that differ at base 9;
  sibling   base 8 not an A, a query k-mer that shares 10 bases and differs at base 10;
  no_sib    base 8 not an A, query k-mers with the key's 9-base prefix that differ at base 9 and no sibling: NO anchor;
  bloom_fp  bases [9, p) all A, the Bloom filter of the query hits by chance, its hashed 11-base bitmap misses, the rule map's
            bit is clear (long query: queued, turned away by the bitmap) - and one with bases [7, p) all A (a candidate at once).

check_branches() asserts from the filters the library's own functions build (tests/pa_rule_map_host.cpp) that every planted key
is in the branch it is named after, and from the model that the rule's anchors exist where they must and nowhere else."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

import pa_cases as PC
import pa_model as M

K = 31
HERE = os.path.dirname(os.path.abspath(__file__))
WINDOWS = ((11, 3000), (13, 10000), (15, 50000))
BLOOM, BITMAP, TAIL_A, RULE, MAP9 = 1, 2, 4, 8, 16
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off"]   # of every build of the shim


def shim(tmp_dir):
    """tests/pa_rule_map_host.cpp as a shared object in tmp_dir, with its prototypes: the one place it is built for ctypes"""
    so = os.path.join(str(tmp_dir), "libpa_rule_map_host.so")
    subprocess.check_call(["g++", "-O2", "-g"] + FLAGS + ["-fPIC", "-shared", "-o", so, os.path.join(HERE, "pa_rule_map_host.cpp")])
    L = C.CDLL(so)
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.rm_bits_words.argtypes, L.rm_bits_words.restype = [C.c_int], C.c_uint64
    L.rm_filter_log.argtypes, L.rm_filter_log.restype = [C.c_longlong], C.c_int
    L.rm_build.argtypes, L.rm_build.restype = [u64p, C.c_int, C.c_int, C.c_int, u32p], None
    L.rm_parts.argtypes = L.rm_candidate2.argtypes = L.rm_candidate3.argtypes = [u32p, C.c_int, C.c_uint32, C.c_int]
    L.rm_check_exhaustive.argtypes, L.rm_check_exhaustive.restype = [u64p, C.c_int, C.c_int, u32p, C.c_int], C.c_longlong
    L.rm_no_growth.argtypes = [u64p, C.c_int, C.c_int, u32p, C.c_int, C.c_int, C.c_uint64, C.c_longlong, C.POINTER(C.c_longlong)]
    L.rm_no_growth.restype = C.c_longlong
    return L


def query_filter(L, seq):
    """(log, bits) of a query's filter as the upload sizes it and k_build_cmp_bits fills it"""
    qi = M.QueryIndex(seq)
    ks = qi.keys.tolist()
    lg = L.rm_filter_log(2 * max(len(seq) - K + 1, 0))
    bits = (C.c_uint32 * int(L.rm_bits_words(lg)))()
    L.rm_build((C.c_uint64 * max(len(ks), 1))(*ks), len(ks), K, lg, bits)
    return lg, bits


def _code(text):
    v = 0
    for c in bytes(text):
        v = (v << 2) | b"ACGT".index(c)
    return v


def _text(v, n):
    return bytes(b"ACGT"[(v >> (2 * (n - 1 - j))) & 3] for j in range(n))


def extend(fx, L, seed=20251021):
    """appends the queries, the genome, the cases and the call "rule" to a fixture of pa_cases.build(); fx["rule_plants"] =
    {case number: [(branch, window position, strand of the search that meets the key, first p bases of the key)]}"""
    rng = random.Random(seed)
    rand, other = PC.rand, PC._other
    keys = {}   # p -> [(branch, 31-mer)]
    qk = []
    for p, _ in WINDOWS:
        ks = []
        for branch, w78 in (("all7", b"AA"), ("base8_A", b"CA"), ("base8_A", b"TA"), ("sibling", b"CG"), ("sibling", b"AT"),
                            ("no_sib", b"GC"), ("no_sib", b"AC")):
            k = rand(rng, 7) + w78 + b"A" * (p - 9) + rand(rng, K - p)
            ks.append((branch, k))
            shares = {"all7": (7, 8), "base8_A": (9,), "sibling": (10,), "no_sib": (9,)}[branch]
            for share in shares:   # pairs that share a few bases more with each other: tree nodes with short edges
                stem = k[:share] + bytes([other(rng, k[share])]) + rand(rng, rng.randrange(3))
                qk.append(stem + rand(rng, K - len(stem)))
                qk.append(stem + rand(rng, K - len(stem)))
        keys[p] = ks
    q_short = b"".join(k + rand(rng, 3) for k in qk)
    while True:   # (the unrelated bases must not hold a sibling of a no_sib key by chance: 1 in 40 does)
        q_long = q_short + rand(rng, 16500)
        p11 = set((M.QueryIndex(q_long).keys >> np.uint64(40)).tolist())
        if not any((_code(k[:9]) << 4 | sib) in p11 for ks in keys.values() for branch, k in ks if branch == "no_sib" for sib in (1, 2, 3)):
            break
    assert len(q_short) < 8000 and len(q_long) >= 16415
    qs = [len(fx["queries"]), len(fx["queries"]) + 1]
    fx["queries"] += [q_short, q_long]
    filt = [query_filter(L, q_short), query_filter(L, q_long)]
    assert filt[0][0] <= 19 < filt[1][0]
    for p, _ in WINDOWS:   # Bloom false positives of either query among the keys X + A..: bitmap miss, rule bit clear / bases [7, p) all A
        for lg, bits in filt:
            want = {"bloom_fp": 1, "bloom_fp_all7": 1}
            p9 = rng.randrange(1 << 18)
            for _ in range(1 << 18):
                p9 = (p9 + 1) & 0x3ffff
                parts = L.rm_parts(bits, lg, p9 << (2 * (p - 9)), p)
                if parts & (BLOOM | BITMAP | MAP9) != BLOOM:
                    continue
                name = "bloom_fp_all7" if p9 & 15 == 0 else "bloom_fp" if not parts & RULE and p9 & 3 else None
                if name and want[name]:
                    want[name] = 0
                    keys[p].append((name, _text(p9, 9) + b"A" * (p - 9) + rand(rng, K - p)))
                if not any(want.values()):
                    break
            assert not any(want.values()), (p, lg)
    g = len(fx["genomes"])
    buf = bytearray(rand(rng, 500))
    first = len(fx["cases"])
    fx["rule_plants"] = {}
    for p, wlen in WINDOWS:
        text = bytearray(rand(rng, wlen))
        plants = []
        n = 2 * len(keys[p])
        for j, (branch, k) in enumerate(keys[p]):
            for strand in (0, 1):   # the key itself: strand 0 of the search meets it; its reverse complement: strand 1 does
                at = 100 + (wlen - 300) * (2 * j + strand) // n
                text[at:at + K] = M.revcomp_text(k) if strand else k
                plants.append((branch, at, strand, _code(k[:p])))
        for rc in (0, 1):
            while len(buf) % 32 != (3 * p + 17 * rc) % 32:
                buf += rand(rng, 1)
            tb = len(buf)
            buf += M.revcomp_text(bytes(text)) if rc else bytes(text)
            for which, q in enumerate(qs):
                fx["rule_plants"][len(fx["cases"])] = plants
                fx["cases"].append(PC.Case("rule_p%d_%s_rc%d" % (p, ("short", "long")[which], rc), "rule", q, 0, len(fx["queries"][q]) - 1,
                                           g, tb, wlen, rc, ()))
    buf += rand(rng, 200)
    fx["genomes"].append(("PA_rule", [("PA_rule_c", bytes(buf))]))
    fx["calls"]["rule"] = list(range(first, len(fx["cases"])))
    fx["rule_filters"] = dict(zip(qs, filt))
    return fx


def check_branches(fx, res, L):
    """every planted key is in the branch it is named after under the filter of its case's query; the model owns anchors of the
    partial-prefix rule in every case, none at a no_sib key, none at a bloom_fp key.  Returns {branch: [keys, keys that own an anchor]}"""
    seen = {}
    for n, plants in fx["rule_plants"].items():
        c, r = fx["cases"][n], res[n]
        lg, bits = fx["rule_filters"][c.q]
        assert r.counters["quirk"] > 0, c.name
        for branch, at, strand, f in plants:
            parts = L.rm_parts(bits, lg, f, r.p)
            c2, c3 = L.rm_candidate2(bits, lg, f, r.p), L.rm_candidate3(bits, lg, f, r.p)
            own = (at, strand) in r.owners
            assert parts & TAIL_A, (c.name, branch, at)
            if branch.startswith("bloom_fp"):
                # false positives of the OTHER query's Bloom filter are unrelated keys here: only the own ones are held to the name
                mine = parts & BLOOM and not parts & BITMAP
                if mine and branch == "bloom_fp":
                    assert not parts & RULE and (c3 != 0) == (lg <= 19) and not own, (c.name, branch, at)
                if mine and branch == "bloom_fp_all7":
                    assert parts & RULE and c3, (c.name, branch, at)
                if not mine:
                    continue
            else:
                assert parts & MAP9 or branch == "all7", (c.name, branch, at)
                assert bool(parts & RULE) == (branch != "no_sib"), (c.name, branch, at)
                if branch == "no_sib":
                    assert not own, (c.name, at, strand)
                if parts & BLOOM:
                    continue   # (a false positive of the Bloom filter: the key does not come to the rule)
                assert bool(c3) == (branch != "no_sib") and (c2 or not c3), (c.name, branch, at)
            if own:
                assert c3, (c.name, branch, at)
            s = seen.setdefault(branch, [0, 0])
            s[0] += 1
            s[1] += own
    for branch in ("all7", "base8_A", "sibling", "no_sib", "bloom_fp", "bloom_fp_all7"):
        assert seen[branch][0] >= 12, branch   # 3 window classes x 2 orientations x 2 strands, under either query
    assert seen["sibling"][1] > 0 and seen["base8_A"][1] + seen["all7"][1] > 0
    return seen
