"""The pairs across shards without a GPU: the host's part (lexicmap_amd/csrc/lm_pair_cross_plan.h: the seed blob's writer,
parser and validator, the slot union of own and blob records, the merge of the ranks' rows), built into a stand-alone program
under AddressSanitizer and UBSan (tests/pair_cross_host.cpp) and compared with plain Python; declarations, exported symbols
and the Python view."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import pytest

import pair_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "lexicmap_amd", "csrc")

NEW_SYMBOLS = ("lm_index_pair_seeds", "lm_index_genome_pairs_across", "lm_pairs_from_rows", "lm_pairs_merge")
HEAD = 56


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_cross") / "pair_cross_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "pair_cross_host.cpp")])

    def run(*cmds):
        r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
        return r.stdout.split("\n")[:len(cmds)]
    return run


def _blob_cmd(k, M, masks, fp, recs, offsets, entries):
    """recs: [(key, idlen, idchar)]; offsets: [ns + 1]; entries: [(kmer, rec)]"""
    return "blob %d %d %d %d %d %d %s %s %d %s" % (k, M, masks, len(offsets) - 1, fp, len(recs), " ".join("%d %d %s" % r for r in recs),
                                                    " ".join(map(str, offsets)), len(entries), " ".join("%d %d" % e for e in entries))


def _py_blob(k, M, masks, fp, recs, offsets, entries):
    """the documented layout, written by struct"""
    ids = b"".join(c.encode() * n for _, n, c in recs)
    out = struct.pack("<Qiiii", 0x3144455352504d4c, k, M, masks, len(offsets) - 1) + struct.pack("<Qqqq", fp, len(recs), len(entries), len(ids))
    out += b"".join(struct.pack("<Q", r[0]) for r in recs) + b"".join(struct.pack("<H", r[1]) for r in recs) + ids
    out += b"".join(struct.pack("<q", o) for o in offsets)
    out += b"".join(struct.pack("<Q", e[0]) for e in entries) + b"".join(struct.pack("<I", e[1]) for e in entries)
    return out


SMALL = dict(k=31, M=70, masks=64, fp=0xfeedfacecafebeef, recs=[(3, 2, "a"), (9, 0, "b"), (1 << 40, 5, "c")], offsets=[0, 2, 2, 5],
             entries=[(11, 0), (1 << 61, 2), (5, 1), (5, 2), (77, 0)])


def _parse_answer(line):
    head, hd, recs, offs, ents = [x.strip() for x in line.split("|")]
    return head.split(), [int(x) for x in hd.split()], recs.split(), [int(x) for x in offs.split()], ents.split()


def test_blob_round_trip_and_its_documented_layout(host):
    cases = [SMALL,
             dict(k=21, M=64, masks=0, fp=1, recs=[], offsets=[0] * 65, entries=[]),                       # no records: a valid empty blob
             dict(k=10, M=64, masks=64, fp=2, recs=[(0, 65535, "z"), (1, 0, "q"), (2, 1, "y")], offsets=[0, 1], entries=[((1 << 20) - 1, 2)]),
             dict(k=32, M=100, masks=0, fp=(1 << 64) - 1, recs=[(5, 3, "g")], offsets=[0, 0, 3, 3], entries=[((1 << 64) - 1, 0), (0, 0), (7, 0)])]
    rng = random.Random(5)
    nrec = 40
    offs = sorted(rng.randrange(0, 300) for _ in range(15))
    cases.append(dict(k=31, M=80, masks=0, fp=99, recs=[(i * 7 + 1, rng.randrange(0, 9), "abcdefgh"[i % 8]) for i in range(nrec)],
                      offsets=[0] + offs + [300], entries=[(rng.getrandbits(62), rng.randrange(nrec)) for _ in range(300)]))
    out = host(*[_blob_cmd(**c) for c in cases])
    for c, line in zip(cases, out):
        head, hd, recs, offs, ents = _parse_answer(line)
        exp = _py_blob(**c)
        assert head[0] == "ok" and int(head[1]) == len(exp)
        if len(exp) <= 4096:
            assert bytes.fromhex(head[2]) == exp
        assert hd == [c["k"], c["M"], c["masks"], len(c["offsets"]) - 1, c["fp"], len(c["recs"]), len(c["entries"])]
        assert recs == ["%d:%d:%s" % (k, n, (ch * 2 if n else "")) for k, n, ch in c["recs"]]
        assert offs == c["offsets"] and ents == ["%d:%d" % e for e in c["entries"]]
    assert int(out[2].split()[1]) == HEAD + 3 * 10 + 65536 + 2 * 8 + 12                                      # ids of 65535, 0 and 1 bytes
    # an id that does not fit 16 bits is refused by the writer
    assert host(_blob_cmd(31, 64, 64, 0, [(1, 65536, "x")], [0, 0], []))[0].startswith("refused")
    # 12 B per entry, 10 B and the id per record
    a = len(_py_blob(**SMALL))
    assert a == HEAD + 3 * 10 + 7 + 4 * 8 + 5 * 12


def test_every_truncation_and_every_single_field_corruption_is_refused_with_a_text(host):
    good = _py_blob(**SMALL)
    assert host("parse " + good.hex(), "parsecopy " + good.hex()) == ["ok 3 5"] * 2
    cmds = ["parsecopy " + (good[:n].hex() or "-") for n in range(len(good))]
    cmds += ["parsecopy " + (good + b"\0" * n).hex() for n in (1, 8)]
    for line in host(*cmds):
        assert line.startswith("refused ") and len(line) > 12, line
    # every field of the blob set to values that break it: the header's numbers, keys, id lengths, offsets, record indexes
    nrec, ns, nent = 3, 3, 5
    o_keys, o_len = HEAD, HEAD + nrec * 8
    o_off = o_len + nrec * 2 + 7
    o_rec = o_off + (ns + 1) * 8 + nent * 8
    fields = [(0, 8), (8, 4), (12, 4), (16, 4), (20, 4), (32, 8), (40, 8), (48, 8)]                          # all of the header but the fingerprint
    fields += [(o_keys + 8 * i, 8) for i in range(nrec)] + [(o_len + 2 * i, 2) for i in range(nrec)]
    fields += [(o_off + 8 * i, 8) for i in range(ns + 1)] + [(o_rec + 4 * i, 4) for i in range(nent)]
    cmds, what = [], []
    for off, size in fields:
        old = int.from_bytes(good[off:off + size], "little")
        for new in {0, 1, old + 1, old - 1 if old else 5, (1 << (8 * size)) - 1, 1 << (8 * size - 1), (1 << (8 * size - 1)) - 1}:
            new &= (1 << (8 * size)) - 1
            if new != old:
                cmds.append("parsecopy " + (good[:off] + new.to_bytes(size, "little") + good[off + size:]).hex())
                what.append((off, size, old, new))
    out = host(*cmds)
    # what a blob alone cannot show as wrong: another k in range, more masks in the index, another selection, a key that still
    # ascends, a record index that is still a record, an offset that stays between its neighbours
    harmless = 0
    for (off, size, old, new), line in zip(what, out):
        ok_allowed = ((off == 8 and 1 <= new <= 32) or (off == 12 and ns <= new < (1 << 31)) or (off == 16 and new < (1 << 31)) or
                      (o_keys <= off < o_len) or (o_off < off < o_off + ns * 8) or (off >= o_rec and new < nrec))
        if line.startswith("ok"):
            assert ok_allowed, (off, size, old, new)
            harmless += 1
        else:
            assert line.startswith("refused ") and len(line) > 12, line
    assert harmless < len(out) // 3
    swapped = dict(SMALL, offsets=[0, 5, 2, 5])                                                              # one offset swapped
    keys_desc = dict(SMALL, recs=[(9, 2, "a"), (3, 0, "b"), (1 << 40, 5, "c")])
    keys_same = dict(SMALL, recs=[(3, 2, "a"), (3, 0, "b"), (1 << 40, 5, "c")])
    rec_out = dict(SMALL, entries=SMALL["entries"][:4] + [(77, 3)])
    last_off = dict(SMALL, offsets=[0, 2, 2, 4])
    first_off = dict(SMALL, offsets=[1, 2, 2, 5])
    words = ("monotone", "ascending", "ascending", "names record", "mask offsets", "mask offsets")
    for line, word in zip(host(*["parse " + _py_blob(**c).hex() for c in (swapped, keys_desc, keys_same, rec_out, last_off, first_off)]), words):
        assert line.startswith("refused") and word in line, line


def test_a_blob_against_the_handle_and_the_call(host):
    good = _py_blob(**SMALL).hex()
    s = SMALL
    ns = len(s["offsets"]) - 1
    args = (s["k"], s["M"], s["fp"], s["masks"], ns)
    out = host("fits %s %d %d %d %d %d" % ((good,) + args),
               "fits %s %d %d %d %d %d" % (good, 21, s["M"], s["fp"], s["masks"], ns),
               "fits %s %d %d %d %d %d" % (good, s["k"], 64, s["fp"], s["masks"], ns),
               "fits %s %d %d %d %d %d" % (good, s["k"], s["M"], s["fp"] ^ 1, s["masks"], ns),
               "fits %s %d %d %d %d %d" % (good, s["k"], s["M"], s["fp"], 256, ns),
               "fits %s %d %d %d %d %d" % (good, s["k"], s["M"], s["fp"], s["masks"], ns + 1))
    assert out[0] == "ok"
    for line, word in zip(out[1:], ("k = 31", "70 masks", "mask values", "masks = 64", "masks = 64")):
        assert line.startswith("refused") and word in line, line
    # the fingerprint: FNV-1a over the count and the values; order and every value count
    def fnv(vals):
        h = 0xcbf29ce484222325
        for v in [len(vals)] + list(vals):
            for b in range(8):
                h = ((h ^ ((v >> (8 * b)) & 0xff)) * 0x100000001b3) & ((1 << 64) - 1)
        return h
    sets = [[], [0], [5, 9, 1 << 61], [9, 5, 1 << 61], [5, 9, (1 << 61) + 1], [5, 9]]
    got = [int(x) for x in host(*["fingerprint %d %s" % (len(m), " ".join(map(str, m))) for m in sets])]
    assert got == [fnv(m) for m in sets] and len(set(got)) == len(sets)


def test_slot_union_is_ascending_and_overlaps_are_detected(host):
    rng = random.Random(17)
    cmds, cases = [], []
    for _ in range(40):
        nb = rng.choice([0, 1, 2, 5])
        pool = rng.sample(range(1, 400), rng.randrange(0, 60))
        lists = [[] for _ in range(nb + 1)]
        for key in pool:
            lists[rng.randrange(nb + 1)].append(key << rng.choice([0, 0, 17]))
        lists = [sorted(set(l)) for l in lists]
        if len({x for l in lists for x in l}) != sum(map(len, lists)):
            continue
        cases.append(lists)
        cmds.append("union %d %s %d %s" % (len(lists[0]), " ".join(map(str, lists[0])), nb,
                                           " ".join("%d %s" % (len(l), " ".join(map(str, l))) for l in lists[1:])))
    assert len(cases) > 25
    for lists, line in zip(cases, host(*cmds)):
        slots, own, blobs = line.split("|")
        slots = [tuple(int(x) for x in s.split(":")) for s in slots.split()]
        exp = sorted((key, src - 1, i) for src, l in enumerate(lists) for i, key in enumerate(l))
        assert slots == exp and [s[0] for s in slots] == sorted(s[0] for s in slots)
        at = {key: n for n, (key, _, _) in enumerate(slots)}
        assert [int(x) for x in own.split()] == [at[key] for key in lists[0]]
        assert [[int(x) for x in b.split()] for b in blobs.split(";")[:-1]] == [[at[key] for key in l] for l in lists[1:]]
    out = host("union 3 1 5 9 1 2 4 5", "union 2 1 5 2 2 7 8 2 6 7", "union 0 2 1 3 1 3", "union 2 1 5 1 2 1 5", "union 0 0", "union 1 4 1 0")
    assert out[0].startswith("refused") and "key 5 " in out[0] and "own record" in out[0] and "blob 0" in out[0]
    assert out[1].startswith("refused") and "key 7 " in out[1] and "blob 0" in out[1] and "blob 1" in out[1]
    assert out[2].startswith("refused") and "key 3 " in out[2]
    assert out[3].startswith("refused") and "own record" in out[3]                                          # the handle's own blob
    assert out[4].strip() == "| |" and out[5].split("|")[0].strip() == "4:-1:0"


def test_merge_equals_pythons_sorted_with_ties_at_every_level(host):
    rng = random.Random(23)
    cmds, cases = [], []
    for _ in range(30):
        np_ = rng.choice([0, 1, 2, 3, 8])
        pairs, want = set(), rng.randrange(0, 70)
        while len(pairs) < want:
            a, b = rng.randrange(30), rng.randrange(30)
            if a != b:
                pairs.add((min(a, b), max(a, b)))
        rows = [(a, b, rng.choice([3, 3, 7, 9]), rng.choice([60, 60, 61, 200])) for a, b in pairs]
        parts = [[] for _ in range(np_)]
        for r in rows:
            if np_:
                parts[rng.randrange(np_)].append(r)
        parts = [PM.order(p) for p in parts]
        cases.append(parts)
        cmds.append("merge %d %s" % (np_, " ".join("%d %s" % (len(p), " ".join("%d %d %d %d" % r for r in p)) for p in parts)))
    seen_ties = 0
    for parts, line in zip(cases, host(*cmds)):
        got = [parts[int(x.split(":")[0])][int(x.split(":")[1])] for x in line.split()]
        exp = PM.order([r for p in parts for r in p])
        assert got == exp
        seen_ties += sum(1 for a, b in zip(exp, exp[1:]) if a[2:] == b[2:] and a[0] == b[0])
    assert seen_ties > 20
    rows = PM.order([(1, 2, 9, 200), (1, 3, 9, 200), (2, 3, 9, 200), (4, 5, 3, 60)])
    as_part = lambda p: "%d %s" % (len(p), " ".join("%d %d %d %d" % r for r in p))
    out = host("merge 2 %s %s" % (as_part(rows), as_part([(1, 3, 9, 200)])),                                  # the same pair, the same sums
               "merge 2 %s %s" % (as_part(rows), as_part([(2, 3, 5, 100)])),                                  # ... with other sums: no neighbours
               "merge 1 %s" % as_part(rows[::-1]),                                                            # a part out of order
               "merge 1 %s" % as_part([rows[0], rows[0]]),
               "merge 2 %s %s" % (as_part(rows[:2]), as_part(rows[2:])))
    assert out[0].startswith("refused") and "1 and 3" in out[0] and "twice" in out[0]
    assert out[1].startswith("refused") and "2 and 3" in out[1]
    assert out[2].startswith("refused") and "order" in out[2]
    assert out[3].startswith("refused")
    assert out[4].split() == ["0:0", "0:1", "1:0", "1:1"]


def test_the_cross_plan_header_has_no_hip_types():
    txt = open(os.path.join(CSRC, "lm_pair_cross_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "hip/" not in code and "threadIdx" not in code and "__global__" not in code and "hipStream" not in code
    assert '#include "lm_pair_cross_plan.h"' in open(os.path.join(CSRC, "lm_pairs.hip")).read()
    host_src = open(os.path.join(HERE, "pair_cross_host.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', host_src) == ["../lexicmap_amd/csrc/lm_pair_cross_plan.h"]


def test_new_symbols_are_declared_and_exported_and_the_header_is_c99():
    import lexicmap_amd as la
    la.build_library()
    hdr = os.path.join(ROOT, "include", "lexicmap_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert re.search(r"lm_status\s+lm_index_pair_seeds\s*\(\s*lm_index\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+lm_pair_opt\s*\*\s*\w+\s*,\s*void\s*\*\*\s*\w+\s*,\s*size_t\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"lm_status\s+lm_index_genome_pairs_across\s*\(\s*lm_index\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+void\s*\*\s*const\s*\*\s*\w+\s*,\s*const\s+size_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+lm_pair_opt\s*\*\s*\w+\s*,\s*lm_pairs\s*\*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"lm_status\s+lm_pairs_merge\s*\(\s*const\s+lm_pairs\s*\*\s*const\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,\s*lm_pairs\s*\*\*\s*\w+\s*\)\s*;", txt)
    out = subprocess.check_output(["nm", "-D", "--defined-only", la.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for f in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % f, txt), f
        assert f in exported, f
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_view_matches_the_c_structs_and_the_merge_runs_without_a_gpu(tmp_path):
    import lexicmap_amd as la
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lexicmap_hip.h"\n'
                   'int main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(lm_pair_opt), sizeof(lm_pair_row), sizeof(lm_pair_stats),'
                   ' offsetof(lm_pair_row, genome1), offsetof(lm_pair_row, n_masks), offsetof(lm_pair_stats, tuples)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    A = la.api
    assert got == [C.sizeof(A.PairOpt), C.sizeof(A.PairRow), C.sizeof(A.PairStats), A.PairRow.genome1.offset, A.PairRow.n_masks.offset,
                   A.PairStats.tuples.offset]
    assert hasattr(la.Index, "pairs_across") and hasattr(la.Index, "pair_seeds") and la.merge_pair_rows is A.merge_pair_rows
    # lm_pairs_from_rows / lm_pairs_merge are host-only: the merge of plain rows, names copied
    rows = [dict(key1=a, key2=b, genome1=b"g%d" % a, genome2=b"g%d" % b, n_masks=n, sum_prefix=s)
            for a, b, n, s in PM.order([(1, 2, 9, 200), (1, 3, 9, 200), (2, 3, 9, 200), (4, 5, 3, 60), (0, 9, 9, 201)])]
    tup = lambda rs: [(r["key1"], r["key2"], r["n_masks"], r["sum_prefix"], r["genome1"], r["genome2"]) for r in rs]
    for split in ([rows], [rows[::2], rows[1::2]], [rows[1::2], [], rows[::2]], [[r] for r in rows[::-1]]):
        assert tup(la.merge_pair_rows(split)) == tup(rows)
    assert la.merge_pair_rows([]) == [] and la.merge_pair_rows([[], []]) == []
    with pytest.raises(ValueError) as e:
        la.merge_pair_rows([rows, rows[2:3]])
    assert "twice" in str(e.value)
