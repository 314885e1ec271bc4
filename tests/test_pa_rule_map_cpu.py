"""The rule map of the pseudo-alignment filter without a GPU (lm_pa_filter_preset / lm_pa_filter_set / lm_pa_candidate3,
lm_algos.h; tests/pa_rule_map_host.cpp):
  1. exhaustive equality: for the queries of tests/pa_cases.py (both sides of 16 414 bases) and a few seeded k-mer sets - the empty
     set, a set whose only k-mer is all A, a set that holds a sibling of a key but not the key's own 11-base prefix - every one of
     the 2^18 bits the library's build functions set equals the rule evaluated literally from the exact sets of 11-base and 9-base
     prefixes;
  2. necessity: every (window position, strand) that owns an anchor of pa_model passes lm_pa_candidate3, for p = 11, 13 and 15, with
     the filter sized as the library sizes it (the property test_pa_edges_cpu.py holds lm_pa_candidate2 to);
  3. no growth: on more than 10^6 seeded keys per filter size lm_pa_candidate3 implies lm_pa_candidate2 (both counts printed);
  4. the same build and checks as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import pa_cases as PC
import pa_model as M
import pa_rule_cases as RC

HERE = os.path.dirname(os.path.abspath(__file__))
K = 31


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return RC.shim(tmp_path_factory.mktemp("pa_rule_map"))


def kmer(text):
    v = 0
    for c in text:
        v = (v << 2) | "ACGT".index(c)
    return v


SIB_P9 = kmer("GATTACAGC")   # base 8 is not an A


def named_sets():
    """[(name, k-mers, filter log)]: the sets the rule's terms are told apart by, and seeded random ones of three sizes"""
    rng = random.Random(20251021)
    out = [("empty", [], 13),
           ("only_all_A", [0], 13),
           ("sibling_without_the_key", [kmer("GATTACAGC" + "AG" + "C" * 20)], 13),
           ("prefix9_base8_A", [kmer("GATTACAGA" + "CG" + "T" * 20)], 13),
           ("prefix9_base8_not_A_no_sibling", [kmer("GATTACAGC" + "CA" + "T" * 20)], 13)]
    for n, lg in ((300, 14), (40000, 20), (200000, 22)):
        out.append(("random_%d" % n, [rng.getrandbits(62) for _ in range(n)], lg))
    return out


@pytest.fixture(scope="module")
def sets(lib):
    """[(name, keys array, n, log, bits)] with the filters built: the named sets and every query of pa_cases"""
    fx = PC.build()
    todo = named_sets()
    for q, seq in enumerate(fx["queries"]):
        qi = M.QueryIndex(seq)
        todo.append(("query_%d_len_%d" % (q, len(seq)), qi.keys.tolist(), lib.rm_filter_log(2 * max(len(seq) - K + 1, 0))))
    out = []
    for name, ks, lg in todo:
        keys = (C.c_uint64 * max(len(ks), 1))(*ks)
        bits = (C.c_uint32 * int(lib.rm_bits_words(lg)))()
        lib.rm_build(keys, len(ks), K, lg, bits)
        out.append((name, keys, len(ks), lg, bits))
    return out


def rule_bit(lib, bits, lg, p9):
    w0 = int(lib.rm_bits_words(lg)) - (1 << 13)   # the rule map is the last region of the layout
    return (bits[w0 + (p9 >> 5)] >> (p9 & 31)) & 1


def test_rule_map_equals_the_literal_rule(lib, sets):
    logs = set()
    for name, keys, n, lg, bits in sets:
        nset = lib.rm_check_exhaustive(keys, n, K, bits, lg)
        assert nset >= 0, "%s: bit p9 = %d of the rule map differs from the literal rule" % (name, -1 - nset)
        assert nset >= 1 << 14, name   # bases 7 and 8 both A: always set
        logs.add(lg)
        print("rule map of %-36s n %7d log %2d: %6d of 262144 bits set" % (name, n, lg, nset))
    assert {19, 20} <= logs   # queries on both sides of 16 414 bases
    by = {s[0]: s for s in sets}
    assert lib.rm_check_exhaustive(*[by["empty"][i] for i in (1, 2)], K, by["empty"][4], 13) == 1 << 14
    assert lib.rm_check_exhaustive(*[by["only_all_A"][i] for i in (1, 2)], K, by["only_all_A"][4], 13) == 1 << 14
    # the terms one by one, at the 9-base prefix GATTACAGC / GATTACAGA
    assert rule_bit(lib, by["sibling_without_the_key"][4], 13, SIB_P9) == 1
    assert rule_bit(lib, by["prefix9_base8_not_A_no_sibling"][4], 13, SIB_P9) == 0
    assert rule_bit(lib, by["prefix9_base8_A"][4], 13, SIB_P9 & ~3) == 1
    assert rule_bit(lib, by["empty"][4], 13, SIB_P9) == 0 and rule_bit(lib, by["empty"][4], 13, SIB_P9 & ~15) == 1
    for p in (11, 13, 15):   # and through the predicate: the key GATTACAGC + A.. + anything
        f = SIB_P9 << (2 * (p - 9))
        assert lib.rm_candidate3(by["sibling_without_the_key"][4], 13, f, p) and lib.rm_candidate2(by["sibling_without_the_key"][4], 13, f, p)
        assert not lib.rm_candidate3(by["prefix9_base8_not_A_no_sibling"][4], 13, f, p)
        assert not lib.rm_candidate3(by["sibling_without_the_key"][4], 13, f | 1, p)   # bases [9, p) not all A


def test_owners_of_model_anchors_pass_candidate3(lib, sets):
    fx = PC.build()
    res = PC.run_models(fx)
    by = {s[0]: s for s in sets}
    owners, rule_only = {}, {}
    try:
        for n, c in enumerate(fx["cases"]):
            r = res[n]
            if not r.owners or r.p > 15:
                continue
            _, keys, nk, lg, bits = by["query_%d_len_%d" % (c.q, len(fx["queries"][c.q]))]
            p11 = set((np.asarray(fx["qindex"][c.q].keys) >> np.uint64(2 * (K - 11))).tolist())
            f, rcv = M.kmers(r.text)
            cls = (r.p, 19 if lg == 19 else 20 if lg == 20 else 0)
            for i, strand in r.owners:
                key = int((rcv if strand else f)[i])
                fp = key >> (2 * (K - r.p))
                assert lib.rm_candidate3(bits, lg, fp, r.p), (c.name, i, strand)
                owners[cls] = owners.get(cls, 0) + 1
                if (key >> (2 * (K - 11))) not in p11:   # no k-mer shares 11 bases: only the rule map can have passed it
                    rule_only[r.p] = rule_only.get(r.p, 0) + 1
    finally:
        for q in fx["qindex"].values():
            q.close()
    print("necessity of lm_pa_candidate3: owners by (p, filter class)", sorted(owners.items()), "owned through the rule map alone", sorted(rule_only.items()))
    for p in (11, 13, 15):
        assert rule_only.get(p, 0) > 0, p
        assert sum(v for (pp, _), v in owners.items() if pp == p) > 50, p
    assert sum(v for (_, cl), v in owners.items() if cl == 19) > 50 and sum(v for (_, cl), v in owners.items() if cl == 20) > 50


def test_candidate3_implies_candidate2(lib, sets):
    seen = set()
    for name, keys, n, lg, bits in sets:
        if lg in seen:
            continue   # one set per filter size
        seen.add(lg)
        tot = [0, 0, 0]
        for p in (11, 13, 15):
            out = (C.c_longlong * 2)()
            bad = lib.rm_no_growth(keys, n, K, bits, lg, p, 7 * lg + p, 400000, out)
            assert bad == 0, "%s, p %d: %d keys pass lm_pa_candidate3 and not lm_pa_candidate2" % (name, p, bad)
            assert out[1] <= out[0]
            tot = [tot[0] + 400000, tot[1] + out[0], tot[2] + out[1]]
        print("no growth, %-36s log %2d: of %d keys lm_pa_candidate2 passes %d, lm_pa_candidate3 %d" % (name, lg, tot[0], tot[1], tot[2]))
    assert {13, 19, 20} <= seen


def test_under_the_sanitizers(lib, sets, tmp_path):
    exe = str(tmp_path / "pa_rule_map_main")
    subprocess.check_call(["g++", "-O1", "-g"] + RC.FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(HERE, "pa_rule_map_main.cpp")])
    inp = tmp_path / "sets.bin"
    with open(inp, "wb") as fh:
        fh.write(struct.pack("=i", len(sets)))
        for _, keys, n, lg, _ in sets:
            fh.write(struct.pack("=ii", n, lg))
            fh.write(bytes(keys)[:8 * n])
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    assert len(r.stdout.strip().split("\n")) == len(sets)
