"""lm_index_screen_genomes without a GPU: the host's part (lexicmap_amd/csrc/lm_screen_plan.h: query layout and regions,
window cuts, piece planning, the merge of partial sums, chunk merge, tie order and cut), built into a stand-alone program
under AddressSanitizer and UBSan (tests/screen_plan_host.cpp) and compared with the Python model (tests/screen_model.py) on
small tables; the model's own self-check on the fixture index; declarations, exported symbols and the Python view."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import genome_build_fixture as F
import oracle as O
import screen_model as SM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "lexicmap_amd", "csrc")

NEW_SYMBOLS = ("lm_screen_opt_default", "lm_index_screen_genomes", "lm_screen_rows", "lm_screen_keys", "lm_screen_prefixes",
               "lm_screen_get_stats", "lm_screen_free", "lm_format_screen_row", "lm_screen_header", "lm_index_screen_structure",
               "lm_index_screen_add_structure")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("screen_plan") / "screen_plan_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "screen_plan_host.cpp")])

    def run(*cmds):
        r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
        return r.stdout.split("\n")[:len(cmds)]
    return run


def test_window_cuts_equal_the_models(host):
    k = 31
    cases = [(1000, 1), (1000, 3), (1001, 3), (1003, 4), (100, 1), (100, 7), (100, 40), (31, 2), (5, 9), (0, 1), (0, 3),
             (2 ** 28 - 1, 1), (2 ** 28 - 1, 1000), (123457, 11)]   # len not divisible, windows = 1, windows > len / k
    out = host(*["windows %d %d" % c for c in cases])
    for (n, w), line in zip(cases, out):
        exp = SM.windows_of(n, w)
        assert line.split() == ["%d:%d" % (s, e - s) for s, e in exp], (n, w, line)
        assert exp[-1][1] == n and len(exp) == w
    assert any(e - s < k for s, e in SM.windows_of(100, 40))   # (windows shorter than k were among the cases)
    assert SM.windows_of(1000, 1) == [(0, 1000)] and SM.windows_of(1003, 4) == [(0, 400), (200, 600), (400, 800), (600, 1003)]


def test_query_layout_and_regions_equal_the_models(host):
    rng = random.Random(5)
    cases = [[100], [60000, 25, 1200, 40000], [10, 0, 10], [0], [31, 31], [1, 1, 1, 1, 1]]
    for k in (21, 31, 32):
        out = host(*["layout %d %d %s" % (k, len(c), " ".join(map(str, c))) for c in cases])
        for c, line in zip(cases, out):
            contigs = [("c%d" % i, bytes(rng.choice(b"ACGTNacgtnYKR") for _ in range(n))) for i, n in enumerate(c)]
            seq, regions = SM.query_layout(contigs, k)
            head, regs = line.split("|")
            head = [int(x) for x in head.split()]
            assert head[0] == len(seq), (k, c)
            starts, pos = [], 0
            for i, n in enumerate(c):
                pos += k if i else 0
                starts.append(pos)
                pos += n
            assert head[1:] == starts
            assert regs.split() == ["%d:%d" % r for r in regions]
            assert regions == [(s - k, s - 1) for s in starts[1:]]          # exactly the spacers, k bases each
            assert not set(seq) - set(b"ACGT") and all(seq[s:e + 1] == b"A" * k for s, e in regions)
    # N and n became A before any gap was looked for: no region for a run of N, unlike the builder's regions
    g3 = dict(F.genomes())["G3"]
    assert SM.query_layout(g3, 31)[1] == [] and len(SM.query_layout(g3, 31, n_runs_skipped=True)[1]) == 4


def test_piece_planning(host):
    rng = random.Random(7)
    cases = []
    for _ in range(40):
        M = rng.choice([1, 2, 5, 64])
        counts = [rng.choice([0, 0, 1, 3, 10, 50]) for _ in range(M)]
        cases.append((rng.choice([1, 4, 25, 10 ** 6]), rng.choice([9, 60, 10 ** 6]), counts))
    out = host(*["pieces %d %d %d %s" % (s, h, len(c), " ".join(map(str, c))) for s, h, c in cases])
    seen_bad = seen_multi = False
    for (soft, hard, counts), line in zip(cases, out):
        if max(counts) > hard:
            assert line.split() == ["bad", str(next(m for m, c in enumerate(counts) if c > hard))]
            seen_bad = True
            continue
        pieces = [tuple(int(x) for x in p.split(":")) for p in line.split()]
        # whole masks, in order, nothing lost; within `soft` unless one mask alone is more; no piece could take the next mask
        assert sum(p[2] for p in pieces) == sum(counts)
        at = 0
        for i, (m0, m1, n) in enumerate(pieces):
            assert m0 >= at and m1 > m0 and n == sum(counts[m0:m1]) and n > 0
            assert not any(counts[at:m0])
            nz = [c for c in counts[m0:m1] if c]
            assert n <= soft or len(nz) == 1
            if i + 1 < len(pieces):
                assert n + next(c for c in counts[m1:] if c) > soft
            at = m1
        assert not any(counts[at:])
        seen_multi |= len(pieces) > 3
    assert seen_bad and seen_multi


def test_partial_sums_of_pieces_add_up(host):
    rng = random.Random(11)
    parts = [(rng.randrange(3), rng.randrange(4), rng.randrange(1, 500), rng.randrange(1, 90), rng.randrange(1, 300), rng.randrange(1, 9))
             for _ in range(60)]
    line = host("partials %d %s" % (len(parts), " ".join(" ".join(map(str, p)) for p in parts)))[0]
    exp = {}
    for i, (q, l, sc, s2, hk, hm) in enumerate(parts):
        e = exp.setdefault((q, l), [0, 0, 0, 0, []])
        for j, x in enumerate((sc, s2, hk, hm)):
            e[j] += x
        e[4].append(i)
    got = [x.split(":") for x in line.split()]
    assert [(int(g[0]), int(g[1])) for g in got] == sorted(exp)
    for g in got:
        e = exp[(int(g[0]), int(g[1]))]
        assert [int(x) for x in g[2:6]] == e[:4] and [int(x) for x in g[6].split(",")] == e[4]   # entries in piece order


def test_chunk_merge_tie_order_and_cut_equal_the_models(host):
    rng = random.Random(13)
    for trial in range(30):
        lists = [[3, 4], [9, 10, 11], [20, 22]]
        keys = rng.sample(range(30), rng.randrange(1, 25))
        per_q = []
        for q in range(3):
            per_q.append({key: dict(score=rng.choice([5, 5, 7, 31, 100]), tag=key) for key in rng.sample(keys, rng.randrange(0, len(keys) + 1))})
        top_n = rng.choice([0, 0, 1, 3, 50])
        list_of = {key: i for i, ks in enumerate(lists) for key in ks}
        hits = [(q, key, list_of.get(key, -1), r["score"]) for q in range(3) for key, r in per_q[q].items()]
        rng.shuffle(hits)
        line = host("rows %d %d %s" % (top_n, len(hits), " ".join(" ".join(map(str, h)) for h in hits)))[0]
        exp = []
        for q in range(3):
            for r in SM.merge_order_cut(per_q[q], lists, top_n):
                exp.append("%d:%d:%d:%s" % (q, r["score"], r["tag"], ",".join(map(str, r["keys"]))))
                assert r["tag"] == r["keys"][0] == r["batch_genome"] == min(r["keys"])   # details of the lowest hit key
        assert line.split() == exp, (trial, line, exp)
    # equal scores: ascending key; a list with one hit record is a row of one key; the cut keeps the head
    rows = SM.merge_order_cut({7: dict(score=9), 2: dict(score=9), 4: dict(score=3), 3: dict(score=7)}, [[3, 4], [7, 8]], 0)
    assert [(r["batch_genome"], r["score"], r["keys"]) for r in rows] == [(3, 10, [3, 4]), (2, 9, [2]), (7, 9, [7])]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    gs = F.genomes()
    M = 1024
    masks = (C.c_uint64 * M)()
    O.lib().lmo_gen_masks(F.K, M, 1, masks)
    d = str(tmp_path_factory.mktemp("screen_model") / "oracle.lmi")
    O.build_index(d, gs, O.default_build_opt(chunks=3, max_genome=F.MAX_GENOME, masks=M), masks=list(masks))
    recs = F.records(gs)
    m = SM.Model(d, F.K, list(masks), SM.chunk_lists(recs), {i: r[0] for i, r in enumerate(recs)})
    yield dict(m=m, gs=gs, M=M)
    m.close()


def test_model_self_check_on_the_fixture_index(model):
    """G1 against the fixture set (1024 masks, so that the oracle builds it in seconds): G1 first with every hit mask at its
    full length, its 5 % sibling second; G6 is one row of two keys; a query shorter than k gives nothing"""
    m, gs = model["m"], dict(model["gs"])
    rows = m.screen_one(gs["G1"], details=True, top_n=0)
    assert rows[0]["batch_genome"] == 0 and rows[0]["genome_id"] == "G1" and rows[1]["batch_genome"] == 7
    assert rows[0]["score2"] == F.K * rows[0]["hit_masks"] and rows[0]["hit_masks"] > 0.9 * model["M"]
    assert set(rows[0]["prefixes"]) == {F.K} and rows[0]["score"] >= rows[0]["score2"] > rows[1]["score2"]
    g6 = m.screen_one(gs["G6"], details=True, top_n=1)
    assert len(g6) == 1 and g6[0]["keys"] == [5, 6] and g6[0]["batch_genome"] == 5
    per = m.per_record(gs["G6"])
    assert g6[0]["score"] == per[5]["score"] + per[6]["score"] and g6[0]["score2"] == sum(per[5]["longest"])
    assert m.screen_one([("s", b"ACGTACGTACGTACGTACGT")]) == []
    plain = m.screen_one(gs["G1"], details=False, top_n=0)
    assert [(r["keys"], r["score"]) for r in plain] == [(r["keys"], r["score"]) for r in rows]
    assert all(r["score2"] == r["hit_masks"] == r["hit_kmers"] == 0 and r["prefixes"] == [] for r in plain)
    lines = SM.format_rows([rows[:1]], ["q"], 21, model["M"], extra=True)
    assert lines[0].startswith("q\tG1\t21\t%.4f\t%d\t%d\t31.00\t31,31" % (rows[0]["hit_masks"] / model["M"], rows[0]["hit_masks"], rows[0]["score2"]))


def test_the_plan_header_has_no_hip_types():
    txt = open(os.path.join(CSRC, "lm_screen_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "hip/" not in code and "threadIdx" not in code and "__global__" not in code
    assert '#include "lm_screen_plan.h"' in open(os.path.join(CSRC, "lm_screen.hip")).read()


def test_new_symbols_are_declared_and_exported_and_the_header_is_c99():
    import lexicmap_amd as la
    la.build_library()
    hdr = os.path.join(ROOT, "include", "lexicmap_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert re.search(r"lm_status\s+lm_index_screen_genomes\s*\(\s*lm_index\s*\*\s*\w+\s*,\s*const\s+lm_genome_query\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+lm_screen_opt\s*\*\s*\w+\s*,\s*lm_screen\s*\*\*\s*\w+\s*\)\s*;", txt)
    out = subprocess.check_output(["nm", "-D", "--defined-only", la.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for f in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % f, txt), f
        assert f in exported, f
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_view_matches_the_c_structs(tmp_path):
    import lexicmap_amd as la
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lexicmap_hip.h"\n'
                   'int main(void) { lm_screen_opt o; lm_screen_opt *p = &o; (void)p;\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(lm_screen_opt), sizeof(lm_genome_query), sizeof(lm_screen_row), sizeof(lm_screen_stats),'
                   ' offsetof(lm_screen_row, genome_id), offsetof(lm_screen_row, hit_masks), offsetof(lm_screen_row, prefixes_off), offsetof(lm_screen_stats, ms_capture)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    A = la.api
    assert got == [C.sizeof(A.ScreenOpt), C.sizeof(A.GenomeQuery), C.sizeof(A.ScreenRow), C.sizeof(A.ScreenStats), A.ScreenRow.genome_id.offset,
                   A.ScreenRow.hit_masks.offset, A.ScreenRow.prefixes_off.offset, A.ScreenStats.ms_capture.offset]
    assert hasattr(la.Index, "screen") and hasattr(la, "format_screen_rows") and hasattr(la.Index, "add_screen_structure")
