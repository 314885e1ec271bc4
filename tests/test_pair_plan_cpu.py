"""lm_index_genome_pairs without a GPU: the host's part (lexicmap_amd/csrc/lm_pair_plan.h: mask selection, the required
number of masks, piece planning and its key width, the addition of partial rows with the exact prune, row order, the
formatter), built into a stand-alone program under AddressSanitizer and UBSan (tests/pair_plan_host.cpp) and compared with
the Python model (tests/pair_model.py); the model's own self-check on the two fixture sets (tests/pair_fixture.py);
declarations, exported symbols and the Python view."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import mask_sets as MS
import oracle as O
import pair_fixture as PF
import pair_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "lexicmap_amd", "csrc")

NEW_SYMBOLS = ("lm_pair_opt_default", "lm_index_genome_pairs", "lm_pairs_rows", "lm_pairs_get_stats", "lm_pairs_free",
               "lm_format_pair_row", "lm_pair_header")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pair_plan") / "pair_plan_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "pair_plan_host.cpp")])

    def run(*cmds):
        r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
        return r.stdout.split("\n")[:len(cmds)]
    return run


def test_mask_selection_equals_the_models(host):
    k = 31
    sets = [MS.skewed(k, 1500), MS.skewed(k, 20000), MS.tall_and_tiny(k)]
    seen_refused = seen_skipped = False
    for masks in sets:
        for nm in (0, 64, 256, 1024, 4096, 3, 63, 128, 65, 16, -4):
            line = host("select %d %d %d %s" % (k, nm, len(masks), " ".join(map(str, masks))))[0]
            try:
                exp = PM.select_masks(masks, k, nm) if nm >= 0 else None
            except ValueError:
                exp = None
            if exp is None:
                assert line == "refused", (len(masks), nm, line[:60])
                seen_refused = True
                continue
            got = [int(x) for x in line.split()]
            assert got[0] == len(exp) and got[1:] == exp, (len(masks), nm)
            if nm:
                seen_skipped |= len(exp) < len(masks)
                assert len({m >> (2 * (k - {64: 3, 256: 4, 1024: 5, 4096: 6}[nm])) for m in masks}) == len(exp) <= nm
    assert seen_refused and seen_skipped
    # above the mask count: refused, also where it is a power of 4
    assert host("select 31 1024 99 %s" % " ".join(map(str, MS.tall_and_tiny(k))))[0] == "refused"
    assert host("select 31 4096 1500 %s" % " ".join(map(str, sets[0])))[0] == "refused"
    # masks=1024 on the skewed 1500: 1024 distinct 5-base prefixes, 476 masks skipped
    assert len(PM.select_masks(sets[0], k, 1024)) == 1024 and len(sets[0]) == 1500


def test_required(host):
    cases = [(0.0, 1500), (0.25, 1500), (1.0, 1500), (0.25, 1024), (1.0, 64), (0.25, 1023), (0.3, 10), (0.7, 10), (0.1, 30),
             (0.29, 100), (0.57, 100), (0.58, 100), (1 / 3, 3), (2 / 3, 3), (0.999999, 1000), (1.5, 10), (0.0, 0)]
    out = host(*["required %r %d" % c for c in cases])
    for (f, t), line in zip(cases, out):
        assert int(line) == PM.required(f, t) == int(f * float(t)), (f, t, line)
    # products that land just either side of an integer
    assert PM.required(0.29, 100) == 28 and PM.required(0.57, 100) == 56 and PM.required(0.58, 100) == 57 and PM.required(0.7, 10) == 7


def _bits(n):
    b = 0
    while (1 << b) < n:
        b += 1
    return b


def test_piece_planning(host):
    rng = random.Random(7)
    cases = []
    for _ in range(60):
        ns = rng.choice([1, 2, 5, 64, 300])
        counts = [rng.choice([0, 0, 1, 3, 10, 50]) for _ in range(ns)]
        cases.append((rng.choice([1, 4, 25, 10 ** 6]), rng.choice([9, 60, 10 ** 6]), rng.choice([1, 8, 26, 27, 28, 29]), counts))
    cases.append((10 ** 6, 10 ** 6, 29, [5, 0, 7, 0, 0, 2]))       # 2^29 slots: one-mask pieces only, no mask bits
    cases.append((10, 10 ** 6, 8, [0, 0, 0, 0]))                   # no tuples at all: no piece
    cases.append((10, 100, 8, [3, 50, 3]))                         # one mask above soft alone, within hard
    cases.append((10, 40, 8, [3, 50, 3]))                          # ... above hard: refused, names the mask
    cases.append((10, 40, 30, [1, 1]))                             # two slots of 30 bits and a length do not fit 64 bits
    out = host(*["pieces %d %d %d %d %s" % (s, h, sb, len(c), " ".join(map(str, c))) for s, h, sb, c in cases])
    seen_bad = seen_multi = seen_cap = False
    for (soft, hard, sb, counts), line in zip(cases, out):
        if 2 * sb + 6 > 64:
            assert line.split() == ["bad", "-1"]
            continue
        if max(counts) > hard:
            assert line.split() == ["bad", str(next(m for m, c in enumerate(counts) if c > hard))]
            seen_bad = True
            continue
        pieces = [tuple(int(x) for x in p.split(":")) for p in line.split()]
        if not any(counts):
            assert pieces == []
            continue
        max_masks = 1 << min(64 - 6 - 2 * sb, 30)
        # whole masks, contiguous from 0 to ns, nothing lost; within `soft` unless one mask alone is more; key width <= 64
        assert pieces[0][0] == 0 and pieces[-1][1] == len(counts)
        for i, (s0, s1, n, mb) in enumerate(pieces):
            assert s1 > s0 and n == sum(counts[s0:s1])
            assert i == 0 or s0 == pieces[i - 1][1]
            nz = [c for c in counts[s0:s1] if c]
            assert n <= soft or len(nz) == 1
            assert mb == _bits(s1 - s0) and 2 * sb + mb + 6 <= 64 and s1 - s0 <= max_masks
            if i + 1 < len(pieces):     # no piece could take the next mask
                assert s1 - s0 == max_masks or (counts[s1] > 0 and n + counts[s1] > soft)
                seen_cap |= s1 - s0 == max_masks
        seen_multi |= len(pieces) > 3
    assert seen_bad and seen_multi and seen_cap
    assert out[60].split() == ["0:1:5:0", "1:2:0:0", "2:3:7:0", "3:4:0:0", "4:5:0:0", "5:6:2:0"]
    assert out[62].split() == ["0:1:3:0", "1:2:50:0", "2:3:3:0"]


def test_partial_rows_add_up_and_the_prune_is_exact(host):
    rng = random.Random(11)
    for trial in range(30):
        total = rng.choice([4, 10, 40])
        req = rng.choice([0, 1, 2, total // 2, total, total + 1])
        npieces = rng.choice([1, 2, 4])
        per_piece = total // npieces
        table, model, dropped = [], {}, set()
        for pc in range(npieces):
            left = total - (pc + 1) * per_piece if pc + 1 < npieces else 0
            part = {}
            for _ in range(rng.randrange(0, 25)):
                pair = rng.randrange(12)
                if pair not in part:
                    n = rng.randrange(1, per_piece + 1)
                    part[pair] = (n, rng.randrange(n * 11, n * 31 + 1))
            line = host("add %d %d %d %s %d %s" % (left, req, len(table), " ".join("%d %d %d" % r for r in table), len(part),
                                                     " ".join("%d %d %d" % ((p,) + part[p]) for p in sorted(part))))[0]
            for p, (n, s) in part.items():
                e = model.setdefault(p, [0, 0])
                e[0] += n
                e[1] += s
            # the dict, with the same exact bound: a pair is gone once it cannot reach `req`, and stays gone
            for p, (n, s) in model.items():
                if n + left < req:
                    dropped.add(p)
            table = [tuple(int(x) for x in r.split(":")) for r in line.split()]
            assert table == [(p, model[p][0], model[p][1]) for p in sorted(model) if p not in dropped], (trial, pc)
        # a dropped pair could never have been a row: the rows are those of the plain sum over all pieces
        plain = [(p, n, s) for p, (n, s) in sorted(model.items()) if n >= req]
        assert [r for r in table if r[1] >= req] == plain == table, trial


def test_row_order_with_ties_at_every_level(host):
    rng = random.Random(13)
    rows = [(rng.randrange(1 << 40), rng.choice([3, 3, 7, 9]), rng.choice([60, 60, 61, 200])) for _ in range(80)]
    rows += [(5, 9, 200), (4, 9, 200), (1 << 45, 9, 200), (6, 9, 201), (7, 10, 1)]
    rows = list({r[0]: r for r in rows}.values())
    line = host("order %d %s" % (len(rows), " ".join("%d %d %d" % r for r in rows)))[0]
    got = [tuple(int(x) for x in r.split(":")) for r in line.split()]
    exp = [(a, n, s) for a, _, n, s in PM.order([(p, 0, n, s) for p, n, s in rows])]
    assert got == exp
    assert got[0] == (7, 10, 1) and got[1] == (6, 9, 201)
    tied = [r for r in got if r[1:] == (9, 200)]
    assert len(tied) > 3 and tied == sorted(tied) and tied[:2] == [(4, 9, 200), (5, 9, 200)] and tied[-1] == (1 << 45, 9, 200)
    assert PM.order([(2, 3, 5, 50), (1, 9, 5, 50), (1, 4, 5, 50), (0, 1, 4, 99), (0, 2, 5, 51)]) == \
        [(0, 2, 5, 51), (1, 4, 5, 50), (1, 9, 5, 50), (2, 3, 5, 50), (0, 1, 4, 99)]


def test_formatter_equals_pythons(host):
    cases = [(21, 1500, 1500, 46500, "A", "Acopy"), (21, 1500, 853, 25000, "A", "A2"), (11, 1024, 1, 11, "x", "y"),
             (31, 64, 16, 333, "GCF_000005845.2", "GCF_000006945.2"), (21, 3, 1, 32, "a", "b"), (21, 7, 2, 45, "a", "b")]
    out = host(*["format 256 %d %d %d %d %s %s" % c for c in cases])
    for (p, total, n, s, g1, g2), line in zip(cases, out):
        exp = PM.format_rows([(0, 1, n, s)], {0: g1, 1: g2}, p, total)[0]
        assert line == "%d|%s" % (len(exp), exp)
    assert out[0] == "34|A\tAcopy\t21\t1.0000\t1500\t46500\t31.00"         # n_masks == total
    # the length needed is returned whatever the capacity; the text is cut, never written past the buffer
    exp = PM.format_rows([(0, 1, 853, 25000)], {0: "A", 1: "A2"}, 21, 1500)[0]
    assert host("format 8 21 1500 853 25000 A A2")[0] == "%d|%s" % (len(exp), exp[:7])
    assert host("format 0 21 1500 853 25000 A A2")[0] == "%d|" % len(exp)
    assert host("header")[0] == PM.HEADER


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("pair_model")
    out = {}
    for name, gs, masks, kw in (("P", PF.p_genomes(), PF.p_masks(), dict(max_genome=PF.P_MAX_GENOME)), ("C", PF.c_genomes(), PF.c_masks(), {})):
        d = str(tmp / name)
        O.build_index(d, gs, O.default_build_opt(chunks=3, masks=len(masks), **kw), masks=masks)
        out[name] = PM.Model(d, PF.K, masks)
    return out


def test_model_self_check_on_P(models):
    """the conditions the GPU tests rely on: a fixture that stops exercising a path fails here"""
    m = models["P"]
    names = PF.p_record_names()
    assert len(names) == 11 and names[6] == names[7] == "S"
    lo = m.min_prefix_range()[0]
    r = m.run(21, 0)
    pairs = r["pairs"]
    assert r["total"] == 1500 and pairs[(0, 4)] == [1500, 31 * 1500]                # A and Acopy: every mask, full length
    assert pairs[(0, 1)] == pairs[(1, 4)] and 0.4 < pairs[(0, 1)][0] / 1500 < 0.8    # a tie only the key order breaks
    assert 0.6 < pairs[(6, 8)][0] / 1500 < 0.9                                      # S record 0 and Sx2
    assert not any(7 in p for p in pairs)                                           # the second record of S pairs with nothing
    assert (5, 10) in pairs and pairs[(5, 10)][0] > 300                             # tiny and tiny2
    assert 0.25 < pairs[(0, 9)][0] / 1500 < 0.45 and pairs[(1, 9)][0] / 1500 < 0.25  # half: A above the default fraction, A2 below
    rows = m.rows(21, 0, 0.0)
    assert any(a[2:] == b[2:] for a, b in zip(rows, rows[1:]))                      # rows equal in n_masks and sum_prefix
    for p in (lo, 21):
        n_out, only, mixed = m.structure(p)
        assert n_out > 1000 and only > 100 and mixed == 0                           # outlier-only groups of two records, none mixed
    assert m.run(21, 1024)["total"] == 1024                                         # masks=1024 really skips masks
    assert len(m.rows(21, 1024)) < len(m.rows(21, 1024, 0.0))                       # the default fraction drops pairs


def test_model_self_check_on_C(models):
    m = models["C"]
    for nm, total in ((64, 64), (0, 256)):
        r = m.run(21, nm)
        assert r["total"] == total and r["largest_group"] > 128 and r["same_record"] >= 1
        assert r["tuples"] > 500_000 * (total // 64) * 0.9
        rows = m.rows(21, nm, 0.0)
        assert sum(1 for a, b in zip(rows, rows[1:]) if a[2:] == b[2:]) > 8000       # the clones: ties by the thousand
        assert len(r["pairs"]) >= 130 * 129 // 2
    assert m.structure(21)[2] == 0


def test_the_plan_header_has_no_hip_types():
    txt = open(os.path.join(CSRC, "lm_pair_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "hip/" not in code and "threadIdx" not in code and "__global__" not in code
    assert '#include "lm_pair_plan.h"' in open(os.path.join(CSRC, "lm_pairs.hip")).read()


def test_new_symbols_are_declared_and_exported_and_the_header_is_c99():
    import lexicmap_amd as la
    la.build_library()
    hdr = os.path.join(ROOT, "include", "lexicmap_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert re.search(r"lm_status\s+lm_index_genome_pairs\s*\(\s*lm_index\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+lm_pair_opt\s*\*\s*\w+\s*,\s*lm_pairs\s*\*\*\s*\w+\s*\)\s*;", txt)
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
                   'int main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(lm_pair_opt), sizeof(lm_pair_row), sizeof(lm_pair_stats),'
                   ' offsetof(lm_pair_opt, min_mask_fraction), offsetof(lm_pair_row, genome2), offsetof(lm_pair_row, sum_prefix),'
                   ' offsetof(lm_pair_stats, ms_entries)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    A = la.api
    assert got == [C.sizeof(A.PairOpt), C.sizeof(A.PairRow), C.sizeof(A.PairStats), A.PairOpt.min_mask_fraction.offset,
                   A.PairRow.genome2.offset, A.PairRow.sum_prefix.offset, A.PairStats.ms_entries.offset]
    assert hasattr(la.Index, "pairs") and hasattr(la, "format_pair_rows") and la.PairOpt is A.PairOpt
