"""lm_index_subseqs without a GPU: the host's part (lexicmap_amd/csrc/lm_subseq_plan.h: flanks, the clamps of the contig and
the concatenated form, name resolution, the plan of a call with its statuses and refusals, the blob layout, the piece cuts,
the FASTA formatter), built into a stand-alone
program under AddressSanitizer and UBSan (tests/subseq_plan_host.cpp) and compared with the Python model
(tests/subseq_model.py), whose short form is itself held to the literal restatement of genome.go's SubSeq2 / SubSeq; the
model against the reference's golden rows; declarations, exported symbols and the Python view."""
import ctypes as C
import gzip
import os
import random
import re
import subprocess

import pytest

import genome_build_fixture as F
import subseq_model as SM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "lexicmap_amd", "csrc")
GOLD = os.path.join(HERE, "golden", "demo")

NEW_SYMBOLS = ("lm_subseq_opt_default", "lm_index_subseqs", "lm_index_subseq_rows", "lm_index_genome_seqs", "lm_subseqs_get",
               "lm_subseqs_get_stats", "lm_subseqs_free", "lm_format_subseqs")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("subseq_plan") / "subseq_plan_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "subseq_plan_host.cpp")])

    def run(*cmds):
        r = subprocess.run([exe], input="\n".join(cmds) + "\n", capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr
        return r.stdout.split("\n")[:len(cmds)]
    return run


def _layouts():
    """(sizes, ci): contig ci has every size 1 .. 9, alone, first or second of two, first, second or third of three"""
    for s in range(1, 10):
        a, b = (s * 3) % 9 + 1, (s * 5) % 9 + 1
        yield [s], 0
        yield [s, a], 0
        yield [a, s], 1
        yield [s, a, b], 0
        yield [a, s, b], 1
        yield [b, a, s], 2


def test_clamp_grid_literal_equals_short_form_equals_planner(host):
    interval = 2
    layouts = list(_layouts())
    out = host(*["grid %d %d %s %d" % (interval, len(sz), " ".join(map(str, sz)), ci) for sz, ci in layouts])
    cases = empties = clamped = 0
    for (sizes, ci), line in zip(layouts, out):
        got = line.rstrip(";").split(";")
        contigs = [("c%d" % i, n) for i, n in enumerate(sizes)]
        n_bases = sum(sizes) + interval * (len(sizes) - 1)
        s = sizes[ci]
        at = 0
        for b in range(1, s + 4):
            for e in range(b, s + 4):
                for up in range(s + 4):
                    for down in range(s + 4):
                        for rc in (0, 1):
                            es, ee = SM.flanks(b, e, rc, up, down)
                            lit = SM.subseq2_literal(n_bases, contigs, interval, "c%d" % ci, es - 1, ee - 1)
                            short = SM.contig_window(sizes, ci, interval, es, ee)
                            assert lit[1] == short[1] and lit[2] + 1 == short[2], (sizes, ci, b, e, up, down, rc, lit, short)
                            if short[1]:
                                assert lit[0] == short[0]
                                # inside the contig: a flank never reaches the spacer or a neighbour
                                off = sum(sizes[:ci]) + ci * interval
                                assert off <= short[0] and short[0] + short[1] <= off + s
                            p = got[at].split(",")
                            assert (int(p[1]), int(p[2]), int(p[3])) == (short[1], es, short[2]), (sizes, ci, b, e, up, down, rc)
                            assert short[1] == 0 or int(p[0]) == short[0]
                            at += 1
                            empties += short[1] == 0
                            clamped += ee > s
        assert at == len(got)
        cases += at
    assert cases > 400_000 and empties > 1000 and clamped > 100_000


def test_concatenated_form_and_its_two_deviations(host):
    cmds, exp = [], []
    for n in range(1, 10):
        for es in range(1, n + 4):
            for ee in range(es, n + 6):
                cmds.append("concat %d %d %d" % (n, es, ee))
                exp.append((n, es, ee))
    seen_beyond = 0
    for (n, es, ee), line in zip(exp, host(*cmds)):
        st, src, ln, b, e = (int(x) for x in line.split())
        assert (st, src, ln, e) == SM.concat_window(n, es, ee) and b == es
        lit = SM.subseq_literal(n, es - 1, ee - 1)
        if es <= n:
            assert st == SM.OK and (src, ln) == lit and e == min(ee, n)     # the reference prints end 0 here: we report the clamp
        else:
            assert st == SM.OUT_OF_RANGE and lit[0] >= n and lit[1] == 1    # the reference reads one base behind the record
            seen_beyond += 1
    assert seen_beyond > 20


def test_flanks_swap_on_the_minus_strand(host):
    cases = [(10, 20, 0, 3, 5), (10, 20, 1, 3, 5), (2, 4, 0, 7, 0), (2, 4, 1, 0, 7), (1, 1, 1, 0, 0), (5, 5, 0, 4, 1000)]
    for c, line in zip(cases, host(*["flanks %d %d %d %d %d" % c for c in cases])):
        assert tuple(int(x) for x in line.split()) == SM.flanks(*c)
    assert SM.flanks(10, 20, 0, 3, 5) == (7, 25) and SM.flanks(10, 20, 1, 3, 5) == (5, 23) and SM.flanks(2, 4, 0, 7, 0) == (1, 4)


def test_name_resolution_split_genome_and_duplicate_ids(host):
    m = SM.Model()
    g6 = [m.ids[r] for r in m.records_of("G6")]
    assert g6 == [["G6_x"], ["G6_y", "G6_z"]]
    dup = [["a", "b", "a"]]
    late_dup = [["x"], ["a", "a"], ["a"]]
    cases = [(g6, "G6_x", -1, (0, 0, SM.OK)), (g6, "G6_y", -1, (1, 0, SM.OK)), (g6, "G6_z", -1, (1, 1, SM.OK)),
             (g6, "G6_w", -1, (-1, -1, SM.NO_SEQ)), (g6, None, -1, (0, -1, SM.OK)), (g6, None, 0, (0, 0, SM.OK)),
             (g6, None, 1, (0, -1, SM.NO_SEQ)), (g6, "G6_y", 7, (1, 0, SM.OK)), ([], "G6_x", -1, (-1, -1, SM.NO_GENOME)),
             ([], None, -1, (-1, -1, SM.NO_GENOME)), (dup, "a", -1, (0, -1, SM.NO_SEQ)), (dup, "b", -1, (0, 1, SM.OK)),
             (dup, None, 2, (0, 2, SM.OK)), (late_dup, "a", -1, (1, -1, SM.NO_SEQ)), (late_dup, "x", -1, (0, 0, SM.OK))]
    cmds = ["resolve %d %s %s %d" % (len(recs), " ".join("%d %s" % (len(r), " ".join(r)) for r in recs), sid or "-", idx)
            for recs, sid, idx, _ in cases]
    for (recs, sid, idx, exp), line in zip(cases, host(*cmds)):
        assert tuple(int(x) for x in line.split()) == exp == SM.resolve(recs, sid, idx), (recs, sid, idx)
    # every status has a text of its own
    texts = host(*["status %d" % s for s in range(5)])
    assert len(set(texts)) == 5 and all(texts)


def _plan(host, m, regions, up=0, down=0, ignore=False, local=None):
    """ss_plan - the plan of a whole call - over the records of the model (local: the records this shard holds, the others
    are known as another shard's) -> (refusal text, None) or (None, [(status, record, key, seq_idx, rc, begin, end, src, len)])"""
    recs = [i for i in range(len(m.records)) if local is None or i in local]
    other = [m.keys[i] for i in range(len(m.records)) if i not in recs]
    w = ["plan", m.interval, up, down, int(ignore), len(recs)]
    for i in recs:
        w += [m.keys[i], m.records[i][0], len(m.ids[i])]
        for cid, n in zip(m.ids[i], m.sizes[i]):
            w += [cid, n]
    w += [len(other)] + other + [len(regions)]
    for r in regions:
        w += ["N" if r.get("key") is None else r["key"], r.get("genome_id") or "-", r.get("seq_id") or "-", r.get("seq_idx", -1),
              int(bool(r.get("rc"))), r["begin"], r["end"]]
    line = host(" ".join(map(str, w)))[0]
    if line.startswith("ERR "):
        return line[4:], None
    assert line.startswith("OK ")
    items = [tuple(int(x) for x in p.split(",")) for p in line[3:].rstrip(";").split(";")] if regions else []
    assert len(items) == len(regions)
    return None, [(st, recs[l] if l >= 0 else -1) + tuple(rest) for st, l, *rest in items]


def _plan_equals_model(m, items, exp, what=""):
    for i, ((st, rec, key, ci, rc, b, e, src, n), a) in enumerate(zip(items, exp)):
        assert (st, rc, b, e) == (a["status"], a["rc"], a["begin"], a["end"]), (what, i, items[i], a)
        if st != SM.OK:
            assert n == 0, (what, i)
            continue
        assert (key, ci, n) == (a["key"], a["seq_idx"], len(a["seq"])) and m.keys[rec] == key, (what, i, items[i])
        s = m.concat[rec][src:src + n]
        assert (SM.revcomp(s) if rc else s) == a["seq"], (what, i)


def test_model_on_the_fixture_set(host):
    """the model against plain slices of the input genomes; the planner on the same regions against the model"""
    gs = F.genomes()
    m = SM.Model(gs)
    regions = [dict(genome_id="G6", seq_id="G6_y", begin=1001, end=3000), dict(key=1, seq_idx=0, begin=59_990, end=60_000),
               dict(key=1, begin=59_991, end=60_010), dict(key=2, seq_idx=0, begin=1, end=10), dict(key=99, seq_idx=0, begin=1, end=2),
               dict(genome_id="G9", seq_id="x", begin=1, end=2), dict(key=1, begin=200_000, end=200_001),
               dict(key=1, seq_idx=1, begin=26, end=30), dict(genome_id="G2", seq_id="G2_b", begin=3, end=5, rc=1),
               dict(genome_id="G6", seq_id="G6_z", begin=29_990, end=30_000, rc=1), dict(genome_id="G6", begin=99_990, end=100_010)]
    for up, down in ((0, 0), (1000, 1000), (7, 50)):
        err, items = _plan(host, m, regions, up, down, ignore=True)
        assert err is None
        _plan_equals_model(m, items, m.run(regions, up, down), (up, down))
    _, items = _plan(host, m, regions, ignore=True)
    assert items[7][0] == SM.OK and items[7][8] == 0                                   # begins behind the contig: answered, no bases
    assert items[0][1:4] == (6, 6, 0) and items[10][1:4] == (5, 5, -1)                 # the second / the first record of the split genome
    d = {cid: s for _, contigs in gs for cid, s in contigs}
    tab = lambda s: F.concatenation([("", s)])   # noqa: E731  (the base table)
    assert len(m.records) == 9 and [g for g, _ in m.records].count("G6") == 2
    a = m.one(dict(genome_id="G6", seq_id="G6_y", begin=1001, end=3000))
    assert a["status"] == SM.OK and a["key"] == 6 and a["seq_idx"] == 0 and a["seq"] == d["G6_y"][1000:3000]
    a = m.one(dict(genome_id="G2", seq_id="G2_b", begin=3, end=5, rc=1), 1000, 1000)
    assert (a["begin"], a["end"], a["seq"]) == (1, 25, SM.revcomp(d["G2_b"]))
    a = m.one(dict(key=1, seq_idx=0, begin=59_990, end=60_000), 0, 50)
    assert (a["end"], a["seq"]) == (60_000, d["G2_a"][59_989:])
    a = m.one(dict(key=1, begin=59_991, end=60_010))                                  # concatenated: across the spacer
    assert a["seq"] == d["G2_a"][59_990:] + b"A" * 10 and a["seq_idx"] == -1 and a["seq_id"] is None
    a = m.one(dict(key=2, seq_idx=0, begin=1, end=10))
    assert a["seq"] == b"A" * 7 + tab(d["G3_c"][7:10])                                 # N is stored as A
    assert m.one(dict(key=2, seq_idx=0, begin=30_901, end=30_903))["seq"] == b"CGA"    # YKR through the base table
    assert m.one(dict(key=99, seq_idx=0, begin=1, end=2))["status"] == SM.NO_GENOME
    assert m.one(dict(genome_id="G9", seq_id="x", begin=1, end=2))["status"] == SM.NO_GENOME
    assert m.one(dict(key=6, seq_idx=0, begin=1, end=2), local={0, 3})["status"] == SM.NOT_LOCAL
    assert m.one(dict(key=1, begin=200_000, end=200_001))["status"] == SM.OUT_OF_RANGE
    assert m.one(dict(key=1, seq_idx=1, begin=26, end=30))["seq"] == b""               # begins behind the contig: no bases
    assert [(c, s) for c, s in m.genome_seqs("G6")] == [(c, tab(s)) for c, s in dict(gs)["G6"]]


def test_the_clamp_grid_through_the_plan_of_a_call(host):
    """ss_plan - the path the library takes - on the grid's records: every contig of one, two and three, begin up to size + 3 and
    far behind it, with flanks, both strands.  A region that begins behind its contig's end is answered without bases wherever
    the contig sits in its record, in both ignore_errors modes"""
    layouts = [sz for sz, _ in _layouts()]
    recs = [("g%d" % i, [("c%d_%d" % (i, c), b"A" * n) for c, n in enumerate(sz)]) for i, sz in enumerate(layouts)]
    m = SM.Model(records=recs, interval=2)
    regions = []
    for i, sz in enumerate(layouts):
        for ci, s in enumerate(sz):
            for b in list(range(1, s + 4)) + [s + 1000, 10 ** 12]:
                for e in (b, b + 2, b + s + 5):
                    regions.append(dict(key=i, seq_idx=ci, begin=b, end=e, rc=(b + e) & 1))
                regions.append(dict(genome_id="g%d" % i, seq_id="c%d_%d" % (i, ci), begin=b, end=b + 1, rc=b & 1))
    empties = 0
    for up, down in ((0, 0), (1, 2), (12, 0)):
        exp = m.run(regions, up, down)
        assert all(a["status"] == SM.OK for a in exp)
        for ignore in (False, True):
            err, items = _plan(host, m, regions, up, down, ignore=ignore)
            assert err is None, err
            _plan_equals_model(m, items, exp, (up, down, ignore))
        empties += sum(1 for a in exp if not a["seq"])
    assert len(regions) > 3000 and empties > 1500
    one = SM.Model(records=[("G8", [("G8_c", b"ACGT" * 50)])], keys=[8])                # the reviewer's case: one 200-base record
    for b in (201, 202, 10 ** 15):
        for ignore in (False, True):
            err, items = _plan(host, one, [dict(key=8, seq_idx=0, begin=b, end=b + 3)], ignore=ignore)
            assert err is None and items[0][0] == SM.OK and items[0][8] == 0 and items[0][5:7] == (b, 200), (b, items)


def test_regions_beyond_the_kernels_fields_are_refused(host):
    """the kernel's region holds a 32-bit start and 31 bits of length: the plan refuses what does not fit, in either mode"""
    big = 2 ** 31 - 1

    class Big(SM.Model):                                                                # (a model of sizes only: no bases are made)
        def __init__(self):
            self.records = [("B", None)]
            self.interval = 1000
            self.keys = [0]
            self.ids = [["a", "b", "c"]]
            self.sizes = [[big, big, big]]
    m = Big()
    ok = [dict(key=0, seq_idx=0, begin=1, end=big), dict(key=0, seq_idx=1, begin=1, end=16, rc=1),
          dict(key=0, begin=2 ** 32 - 4, end=2 ** 32 + 9), dict(key=0, begin=2 ** 32, end=2 ** 32),
          dict(key=0, seq_idx=2, begin=big + 5, end=big + 9)]                            # behind its contig: nothing is read
    err, items = _plan(host, m, ok)
    assert err is None and [(x[0], x[7], x[8]) for x in items] == \
        [(0, 0, big), (0, big + 1000, 16), (0, 2 ** 32 - 5, 14), (0, 2 ** 32 - 1, 1), (0, items[4][7], 0)]
    bad = [dict(key=0, begin=1, end=2 ** 31), dict(key=0, seq_idx=1, begin=big - 15, end=big, rc=1), dict(key=0, begin=5, end=3 * big),       # 2^31 bases and more
           dict(key=0, begin=2 ** 32 + 1, end=2 ** 32 + 1), dict(key=0, seq_idx=2, begin=10, end=20)]   # start behind 2^32 - 1 (0-based)
    for r in bad:
        for ignore in (False, True):
            err, items = _plan(host, m, [ok[0], r], ignore=ignore)
            assert items is None and err.startswith("plan: region 1: a region of 2^31 bases or more"), (r, err)


def test_every_refusal_with_and_without_ignore_errors(host):
    m = SM.Model()
    good = dict(key=4, seq_idx=0, begin=11, end=30)
    shard = {0, 3, 4, 5, 6}                                                              # the records of this shard
    bad = [(dict(key=99, seq_idx=0, begin=1, end=5), SM.NO_GENOME, None, "key 99 (batch 0, index 99), sequence number 0, 1-5"),
           (dict(key=(3 << 17) | 7, begin=1, end=5), SM.NO_GENOME, None, "key 393223 (batch 3, index 7), 1-5"),
           (dict(genome_id="G9", seq_id="G9_c", begin=1, end=5), SM.NO_GENOME, None, "genome G9, sequence G9_c, 1-5"),
           (dict(genome_id="G2", seq_id="G2_a", begin=1, end=5), SM.NO_GENOME, shard, "genome G2, sequence G2_a"),   # by name: the shard's own
           (dict(key=1, seq_id="G2_e", begin=1, end=5), SM.NO_SEQ, None, "sequence G2_e"),
           (dict(key=1, seq_idx=4, begin=1, end=5), SM.NO_SEQ, None, "sequence number 4"),                          # beyond the record's contigs
           (dict(genome_id="G6", seq_id="G1_c", begin=1, end=5), SM.NO_SEQ, None, "genome G6, sequence G1_c"),
           (dict(genome_id="G6", seq_idx=1, begin=1, end=5), SM.NO_SEQ, None, "genome G6, sequence number 1"),      # the FIRST record has one
           (dict(key=8, begin=204, end=208), SM.OUT_OF_RANGE, None, "key 8 (batch 0, index 8), 204-208"),
           (dict(key=5, begin=100_005, end=100_005, rc=1), SM.OUT_OF_RANGE, None, "100005-100005"),
           (dict(key=1, seq_idx=0, begin=10, end=400), SM.NOT_LOCAL, shard, "key 1 "),
           (dict(key=8, begin=1, end=5, rc=1), SM.NOT_LOCAL, shard, "key 8 ")]
    status_text = host(*["status %d" % s for s in range(5)])
    for r, st, local, names in bad:
        regions = [good, r, good, r]
        err, items = _plan(host, m, regions, 3, 4, ignore=True, local=local)           # with: the status, no bases, the rest answered
        assert err is None and [x[0] for x in items] == [SM.OK, st, SM.OK, st] and items[1][8] == 0 and items[0][8] == 27, (r, items)
        _plan_equals_model(m, items, m.run(regions, 3, 4, local=local), r)
        err, items = _plan(host, m, regions, 3, 4, ignore=False, local=local)          # without: the first failing region, by number
        assert items is None and err.startswith("plan: region 1 (") and "region 3" not in err, err
        assert names in err and status_text[st] in err and "ignore_errors" in err, err
        assert ("another shard" in err) == (st == SM.NOT_LOCAL), err
    # a contig id that occurs twice in one record: refused, seq_idx names it
    dup = SM.Model(records=[("D", [("a", b"ACGTAC"), ("b", b"CC"), ("a", b"GGT")])], interval=2)
    regions = [dict(genome_id="D", seq_id="a", begin=1, end=2), dict(key=0, seq_id="a", begin=1, end=2), dict(key=0, seq_idx=2, begin=1, end=3),
               dict(genome_id="D", seq_id="b", begin=1, end=2)]
    err, items = _plan(host, dup, regions, ignore=True)
    assert [x[0] for x in items] == [SM.NO_SEQ, SM.NO_SEQ, SM.OK, SM.OK] and items[2][7:] == (12, 3)
    _plan_equals_model(dup, items, dup.run(regions), "dup")
    err, _ = _plan(host, dup, regions)
    assert err.startswith("plan: region 0 (genome D, sequence a, 1-2)") and "seq_idx" in err
    # the arguments: refused with or without ignore_errors, the region by its number
    for ignore in (False, True):
        err, items = _plan(host, m, [good, good, dict(key=4, seq_idx=0, begin=0, end=3)], ignore=ignore)
        assert items is None and err == "plan: region 2: both begin and end position should not be <= 0"
        assert _plan(host, m, [dict(key=4, seq_idx=0, begin=-5, end=-2), good], ignore=ignore)[0].startswith("plan: region 0: both begin")
        assert _plan(host, m, [dict(key=99, begin=0, end=3)], ignore=ignore)[0].startswith("plan: region 0: both begin")   # before any lookup
        assert _plan(host, m, [good, dict(key=4, seq_idx=0, begin=5, end=4)], ignore=ignore)[0] == \
            "plan: region 1: begin position should be <= end position"
        for up, down in ((-1, 0), (0, -1), (-7, -7)):
            assert _plan(host, m, [good], up, down, ignore=ignore) == ("plan: upstream and downstream should be >= 0", None)
        assert _plan(host, m, [], 2, 2, ignore=ignore) == (None, [])
    # the first failure is the one reported: a status at region 1 without ignore_errors, the argument at region 2 with it
    mixed = [good, dict(key=99, begin=1, end=2), dict(key=4, begin=3, end=2)]
    assert _plan(host, m, mixed)[0].startswith("plan: region 1 (key 99 ")
    assert _plan(host, m, mixed, ignore=True)[0].startswith("plan: region 2: begin position")
    assert _plan(host, m, [good, good], ignore=False)[0] is None


def test_layout_offsets_are_multiples_of_16(host):
    rng = random.Random(3)
    cases = [[rng.choice([0, 0, 1, 15, 16, 17, 31, 32, 33, 1000, 4097]) for _ in range(rng.randrange(1, 40))] for _ in range(30)]
    cases += [[], [0], [0, 0, 0]]
    for lens, line in zip(cases, host(*["layout %d %s" % (len(c), " ".join(map(str, c))) for c in cases])):
        goff = [int(x) for x in line.split()]
        exp = [0]
        for n in lens:
            exp.append(exp[-1] + (n + 15) // 16)
        assert goff == exp                      # region i lies at byte 16 * goff[i]: a multiple of 16, regions do not overlap
        assert all(16 * (goff[i + 1] - goff[i]) >= n for i, n in enumerate(lens))


def _pieces(host, budget, lens):
    line = host("pieces %d %d %s" % (budget, len(lens), " ".join(map(str, lens))))[0]
    return [tuple(int(x) for x in p.split(":")) for p in line.split()]


def test_piece_cuts(host):
    assert _pieces(host, 48, [100]) == [(0, 3, 0, 1), (3, 6, 0, 1), (6, 7, 0, 1)]              # one region over three pieces
    assert _pieces(host, 32, [20, 0, 20]) == [(0, 2, 0, 1), (2, 4, 2, 3)]                      # a zero-length region between two
    assert _pieces(host, 16, [20, 0, 20]) == [(0, 1, 0, 1), (1, 2, 0, 1), (2, 3, 2, 3), (3, 4, 2, 3)]  # a budget of 16 bytes
    assert _pieces(host, 0, [17]) == [(0, 1, 0, 1), (1, 2, 0, 1)]                              # below one group: one group
    assert _pieces(host, 1 << 30, [0, 0]) == [] and _pieces(host, 64, []) == []
    assert _pieces(host, 1 << 30, [0, 5, 0, 40, 0]) == [(0, 4, 1, 4)]
    rng = random.Random(5)
    for _ in range(40):
        lens = [rng.choice([0, 0, 1, 16, 17, 40, 100, 1000]) for _ in range(rng.randrange(1, 30))]
        budget = rng.choice([16, 32, 100, 160, 4096])
        per = max(1, budget // 16)
        goff = [0]
        for n in lens:
            goff.append(goff[-1] + (n + 15) // 16)
        ps = _pieces(host, budget, lens)
        at = 0
        for g0, g1, r0, r1 in ps:
            assert g0 == at and g0 < g1 <= g0 + per
            at = g1
            owners = [i for i in range(len(lens)) if goff[i] < g1 and goff[i + 1] > g0]   # regions with a group in [g0, g1)
            assert r0 == owners[0] and r1 == owners[-1] + 1
        assert at == goff[-1]


def test_the_kernel_lane_on_the_host_reads_only_the_regions_bytes(host):
    """ss_group - the lane of k_subseq_extract - under AddressSanitizer over an allocation that ends with the region's last
    byte: every length around the group and word sizes, every 2-bit phase, both strands, the region's first byte at every
    place of an aligned word"""
    rng = random.Random(17)
    genome = bytes(rng.choice(b"ACGT") for _ in range(1200))
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    packed = bytearray((len(genome) + 3) // 4)
    for i, c in enumerate(genome):
        packed[i >> 2] |= code[c] << ((3 - (i & 3)) << 1)
    cmds, exp = [], []
    for ln in (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023):
        for start in (0, 1, 2, 3, 4, 5, 6, 7, 13, 18, 23, 160):
            for rc in (0, 1):
                m = (start + ln) % 4 if start else 0
                lo, hi = start >> 2, (start + ln - 1) >> 2
                cmds.append("extract %d %d %d %d %s" % (start, ln, rc, m, packed[lo:hi + 1].hex()))
                s = genome[start:start + ln]
                s = SM.revcomp(s) if rc else s
                exp.append(s.decode() + "." * (-ln % 16))
    assert host(*cmds) == exp


def test_formatter_equals_the_models(host):
    rng = random.Random(9)
    seqs = {n: "".join(rng.choice("ACGT") for _ in range(n)) for n in (0, 1, 59, 60, 61, 120, 121, 180)}
    cmds, exp = [], []
    for w in (0, 1, 59, 60, 61, -3):
        for n, s in seqs.items():
            cmds.append("wrap %d %s" % (w, s or "-"))
            exp.append(SM.wrap(s.encode(), w).decode().replace("\n", "|"))
    assert host(*cmds) == exp
    assert SM.wrap(b"A" * 120, 60) == b"A" * 60 + b"\n" + b"A" * 60 and SM.wrap(b"", 60) == b"" and SM.wrap(b"ACG", 0) == b"ACG"
    gold = open(os.path.join(GOLD, "q.gene.fasta.lexicmap_top-2-genomes_all.tsv")).read().split("\n")[1]
    row = "\t".join(gold.split("\t")[:20])
    cases = [("NZ_CP033092.2", 458539, 460130, 0, row + "\tX"), ("NZ_CP033092.2", 1, 9, 1, row), ("G6", 3, 4, 1, None), ("c", 1, 1, 0, None)]
    got = host(*["header %s %d %d %d %s" % (n, b, e, rc, r.replace("\t", "@") if r else "-") for n, b, e, rc, r in cases])
    for (n, b, e, rc, r), line in zip(cases, got):
        assert line == SM.header(n, b, e, rc, r)
    assert got[2] == ">G6:3-4:-"
    assert got[0].startswith(">NZ_CP033092.2:458539-460130:+ query=NC_000913.3:4166659-4168200 sgenome=GCF_003697165.2 sseqid=NZ_CP033092.2 "
                             "qcovGnm=100.000 cls=1 hsp=1 qcovHSP=100.000 alenHSP=1542 pident=99.805 gaps=0 qstart=1 qend=1542 "
                             "sstart=458559 send=460100 sstr=+ slen=4903501 evalue=0.00e+00 bitscore=2767")
    assert got[0].endswith("bitscore=2767")
    # the whole text: a failed region prints nothing, an empty sequence prints an empty line
    ans = [dict(status=0, seq_idx=0, seq_id="c1", genome_id="g", begin=1, end=3, rc=0, seq=b"ACG"),
           dict(status=2, seq_idx=-1, seq_id=None, genome_id="g", begin=1, end=3, rc=0, seq=b""),
           dict(status=0, seq_idx=-1, seq_id=None, genome_id="g", begin=5, end=4, rc=1, seq=b"")]
    assert SM.fasta(ans, 60) == b">c1:1-3:+\nACG\n>g:5-4:-\n\n"


def _read_fasta_gz(path):
    out = []
    for line in gzip.open(path, "rt"):
        if line.startswith(">"):
            out.append([line[1:].split()[0], []])
        else:
            out[-1][1].append(line.strip())
    return [(i, "".join(s).encode()) for i, s in out]


def test_model_reproduces_the_sseq_column_of_the_reference_golden():
    """the 14 rows of the reference's -a golden: sseq without gaps is contig[sstart - 1 : send], reverse-complemented for '-'"""
    recs = [(f[:-6], _read_fasta_gz(os.path.join(GOLD, f))) for f in ("GCF_002949675.1.fa.gz", "GCF_003697165.2.fa.gz")]
    m = SM.Model(records=recs)
    lines = open(os.path.join(GOLD, "q.gene.fasta.lexicmap_top-2-genomes_all.tsv")).read().rstrip("\n").split("\n")[1:]
    assert len(lines) == 14
    strands = set()
    for line in lines:
        c = line.split("\t")
        a = m.one(dict(genome_id=c[3], seq_id=c[4], begin=int(c[14]), end=int(c[15]), rc=c[16] == "-"))
        assert a["status"] == SM.OK and a["seq"].decode() == c[22].replace("-", ""), c[:20]
        assert (a["begin"], a["end"]) == (int(c[14]), int(c[15]))
        strands.add(c[16])
    assert strands == {"+", "-"}


def test_the_plan_header_has_no_hip_types():
    txt = open(os.path.join(CSRC, "lm_subseq_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "hip/" not in code and "threadIdx" not in code and "__global__" not in code
    src = open(os.path.join(CSRC, "lm_subseq.hip")).read()
    assert '#include "lm_subseq_plan.h"' in src and "k_subseq_extract" in src
    assert "lm_subseq.o" in open(os.path.join(CSRC, "Makefile")).read()


def test_new_symbols_are_declared_and_exported_and_the_header_is_c99():
    import lexicmap_amd as la
    la.build_library()
    hdr = os.path.join(ROOT, "include", "lexicmap_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert re.search(r"lm_status\s+lm_index_subseqs\s*\(\s*lm_index\s*\*\s*\w+\s*,\s*const\s+lm_region\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+lm_subseq_opt\s*\*\s*\w+\s*,\s*lm_subseqs\s*\*\*\s*\w+\s*\)\s*;", txt)
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
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(lm_region), sizeof(lm_subseq_opt), sizeof(lm_subseq_info),'
                   ' sizeof(lm_subseq_stats), offsetof(lm_region, begin), offsetof(lm_subseq_info, off), offsetof(lm_subseq_info, seq_id),'
                   ' offsetof(lm_subseq_stats, ms_plan), LM_REGION_BY_NAME == 18446744073709551615ull); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    A = la.api
    assert got == [C.sizeof(A.Region), C.sizeof(A.SubseqOpt), C.sizeof(A.SubseqInfo), C.sizeof(A.SubseqStats), A.Region.begin.offset,
                   A.SubseqInfo.off.offset, A.SubseqInfo.seq_id.offset, A.SubseqStats.ms_plan.offset, 1]
    assert A.REGION_BY_NAME == (1 << 64) - 1
    assert [A.SUBSEQ_OK, A.SUBSEQ_NO_GENOME, A.SUBSEQ_NO_SEQ, A.SUBSEQ_OUT_OF_RANGE, A.SUBSEQ_NOT_LOCAL] == \
        [SM.OK, SM.NO_GENOME, SM.NO_SEQ, SM.OUT_OF_RANGE, SM.NOT_LOCAL]
    for f in ("subseq", "subseq_rows", "genome_seqs"):
        assert hasattr(la.Index, f)
    assert hasattr(la, "format_subseqs") and la.Subseqs is A.Subseqs
