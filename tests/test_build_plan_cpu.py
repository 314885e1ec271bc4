"""The record planner of the genome builder (lexicmap_amd/csrc/lm_build_plan.h) built for the host
(tests/build_plan_host.cpp), against what the oracle's index writer (oracle/lmo_build.c) produces for the fixture set of
tests/genome_build_fixture.py: which contigs form which genome record, record lengths, chunk lists, keys, input bases - and
the new C-ABI declarations (exported, still C99)."""
import ctypes as C
import os
import re
import struct
import subprocess

import pytest

import genome_build_fixture as F
import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "build_plan_host.cpp")
HDR = os.path.join(ROOT, "lexicmap_amd", "csrc", "lm_build_plan.h")
LIB = os.path.join(HERE, "libbuild_plan_host.so")
NEW_SYMBOLS = ["lm_build_opt_default", "lm_index_builder_new", "lm_index_builder_add", "lm_index_builder_finish",
               "lm_index_builder_free", "lm_index_builder_last_error"]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", LIB, SRC])
    lib = C.CDLL(LIB)
    i32p, i64p, u32p = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)
    lib.bp_plan.argtypes = [u32p, C.c_int, C.c_int, C.c_int, C.c_int64, i32p, i32p, i32p, i64p, i32p]
    lib.bp_regions.argtypes = [C.c_char_p, u32p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, i32p, i32p]
    lib.bp_key.argtypes = [C.c_int64, C.c_int]
    lib.bp_key.restype = C.c_uint64
    lib.bp_keeps.argtypes = [C.c_int64, C.c_int, C.c_int]
    lib.bp_base_code.argtypes = [C.c_int]
    lib.bp_base_code.restype = C.c_uint
    lib.bp_slot_bytes.argtypes = [C.c_int32]
    lib.bp_slot_bytes.restype = C.c_int64
    return lib


def plan(L, lens, k=31, interval=1000, max_genome=F.MAX_GENOME):
    """records as (first, n, len, bases, [dst_off of its contigs]) or the negative reason"""
    nc = len(lens)
    arr = (C.c_uint32 * max(nc, 1))(*lens)
    first, n, ln = [(C.c_int32 * (nc + 1))() for _ in range(3)]
    bases = (C.c_int64 * (nc + 1))()
    dst = (C.c_int32 * max(nc, 1))()
    r = L.bp_plan(arr, nc, k, interval, max_genome, first, n, ln, bases, dst)
    if r < 0:
        return r
    return [(first[i], n[i], ln[i], bases[i], [dst[first[i] + c] for c in range(n[i])]) for i in range(r)]


def regions(L, contigs, rec, k=31, interval=1000, max_genome=F.MAX_GENOME):
    lens = [len(s) for _, s in contigs]
    arr = (C.c_uint32 * len(lens))(*lens)
    cap = 4096
    s, e = (C.c_int32 * cap)(), (C.c_int32 * cap)()
    n = L.bp_regions(b"".join(bytes(x) for _, x in contigs), arr, len(lens), k, interval, max_genome, rec, cap, s, e)
    assert 0 <= n <= cap
    return [(s[i], e[i]) for i in range(n)]


@pytest.fixture(scope="module")
def oracle_index(tmp_path_factory):
    """the fixture set written by the oracle's writer, read back from its files: records, chunk lists, info.toml"""
    d = str(tmp_path_factory.mktemp("plan") / "fix.lmi")
    gs = F.genomes()
    O.build_index(d, gs, O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME, masks=256))
    recs = []
    idx = open(os.path.join(d, "genomes", "batch_0000", "genomes.bin.idx"), "rb").read()
    dat = open(os.path.join(d, "genomes", "batch_0000", "genomes.bin"), "rb").read()
    nrec = struct.unpack(">I", idx[20:24])[0]
    for r in range(nrec):
        off, bases = struct.unpack(">QI", idx[24 + 12 * r:36 + 12 * r])
        p = off
        il = struct.unpack(">H", dat[p:p + 2])[0]
        gid = dat[p + 2:p + 2 + il].decode()
        p += 2 + il
        gsize, ln, nseqs = struct.unpack(">III", dat[p:p + 12])
        p += 12
        sizes, ids = [], []
        for _ in range(nseqs):
            sz, sl = struct.unpack(">IH", dat[p:p + 6])
            ids.append(dat[p + 6:p + 6 + sl].decode())
            sizes.append(sz)
            p += 6 + sl
        assert ln == bases
        recs.append(dict(id=gid, genome_size=gsize, len=ln, nseqs=nseqs, seq_sizes=sizes, seq_ids=ids))
    cb = open(os.path.join(d, "genomes.chunks.bin"), "rb").read()
    lists, p = [], 0
    while p < len(cb):
        n = struct.unpack(">Q", cb[p:p + 8])[0]
        lists.append(list(struct.unpack(">%dQ" % n, cb[p + 8:p + 8 + 8 * n])))
        p += 8 + 8 * n
    info = open(os.path.join(d, "info.toml")).read()
    return dict(recs=recs, lists=lists, input_bases=int(re.search(r"input-bases = (\d+)", info).group(1)),
                input_genomes=int(re.search(r"input-genomes = (\d+)", info).group(1)), genomes=gs)


def test_records_of_the_fixture_set_equal_the_oracle_writers(L, oracle_index):
    exp = oracle_index["recs"]
    got, lists, nrec, bases = [], [], 0, 0
    for gid, contigs in oracle_index["genomes"]:
        recs = plan(L, [len(s) for _, s in contigs])
        assert isinstance(recs, list), (gid, recs)
        keys = []
        for first, n, ln, b, dst in recs:
            got.append(dict(id=gid, genome_size=b, len=ln, nseqs=n, seq_sizes=[len(s) for _, s in contigs[first:first + n]],
                            seq_ids=[c for c, _ in contigs[first:first + n]]))
            keys.append(L.bp_key(nrec, 5000))
            nrec += 1
            bases += b
            # every contig lies where the concatenation has it, spacers between
            at = 0
            for c in range(n):
                at += 1000 if c else 0
                assert dst[c] == at
                at += len(contigs[first + c][1])
            assert at == ln
        if len(keys) > 1:
            lists.append(keys)
    assert len(got) == len(exp) == 9
    assert got == exp
    assert lists == oracle_index["lists"] == [[5, 6]]
    assert bases == oracle_index["input_bases"] and oracle_index["input_genomes"] == 8
    assert [(r["id"], r["nseqs"]) for r in got[5:7]] == [("G6", 1), ("G6", 2)]


def test_split_rule_and_refusals(L):
    # a contig that would take the concatenation (spacers included) past max_genome starts the next record
    assert [(f, n, ln) for f, n, ln, _, _ in plan(L, [100, 100, 100], max_genome=1200, interval=1000)] == [(0, 2, 1200), (2, 1, 100)]
    # the spacer in front of the contig is not counted when the split is decided (lmo_builder_add: cur + contig_lens[i] > maxg), so a
    # record may pass max_genome by one spacer
    assert [(f, n, ln) for f, n, ln, _, _ in plan(L, [100, 101, 100], max_genome=1200, interval=1000)] == [(0, 2, 1201), (2, 1, 100)]
    assert [(f, n, ln) for f, n, ln, _, _ in plan(L, [100, 1101, 100], max_genome=1200, interval=1000)] == [(0, 1, 100), (1, 1, 1101), (2, 1, 100)]
    assert [(f, n, ln) for f, n, ln, _, _ in plan(L, [600, 600], max_genome=1200, interval=1000)] == [(0, 2, 2200)]
    assert plan(L, []) == -1                                 # no contig
    assert plan(L, [F.MAX_GENOME + 1, 50]) == -2             # "skipping a big genome"
    assert isinstance(plan(L, [F.MAX_GENOME]), list)
    assert plan(L, [5]) == -3 and plan(L, [30]) == -3        # shorter than k
    assert isinstance(plan(L, [31]), list)
    assert isinstance(plan(L, [10, 10], interval=11), list)  # 31 with the spacer
    assert plan(L, [(1 << 28) - 501, 400], max_genome=0) == -4   # joined (the spacer is not counted), 2^28 bases or more with it
    assert [(f, n) for f, n, _, _, _ in plan(L, [1 << 27, 1 << 27], max_genome=0)] == [(0, 1), (1, 1)]
    assert plan(L, [(1 << 28) - 1], max_genome=0)[0][2] == (1 << 28) - 1
    assert plan(L, [1 << 28], max_genome=0) == -2            # max_genome <= 0 means 2^28 - 1
    # a record that is too short refuses the whole genome, whichever record it is
    assert plan(L, [1000, 1000, 5], max_genome=1000) == -3 and plan(L, [5, 1000, 1000], max_genome=1000) == -3


def test_skip_regions_of_the_fixture_set(L):
    gs = dict(F.genomes())
    # G3: N x 7 at 0, N x 5 at 2000, N x 300 at 30000, n x 9 at the end; the run of 4 at 1000 is no region
    assert regions(L, gs["G3"], 0) == [(0, 6), (2000, 2004), (30_000, 30_299), (89_991, 89_999)]
    # G2: three spacers
    assert regions(L, gs["G2"], 0) == [(60_000, 60_999), (61_025, 62_024), (63_225, 64_224)]
    # G6: the first record has none, the second the spacer between y and z
    assert regions(L, gs["G6"], 0) == [] and regions(L, gs["G6"], 1) == [(80_000, 80_999)]
    assert regions(L, gs["G1"], 0) == []
    # against a restatement of the rule on the concatenation: ascending, disjoint, runs of >= 5 only, lower case counts
    contigs = [("a", b"NNNNNACGTnnnnACGTNNNNN"), ("b", b"nNnNnN" + b"ACGT" * 10 + b"NNNN"), ("c", b"N" * 40)]
    cat = (b"-" * 7).join(s for _, s in contigs)
    exp = [(m.start(), m.end() - 1) for m in re.finditer(rb"-+|[Nn]{5,}", cat)]
    got = regions(L, contigs, 0, k=3, interval=7, max_genome=10_000)
    assert got == exp and all(a[1] < b[0] for a, b in zip(got, got[1:]))


def test_keys_shards_base_table_and_slots(L):
    assert L.bp_key(0, 5000) == 0 and L.bp_key(4999, 5000) == 4999 and L.bp_key(5000, 5000) == 1 << 17
    assert [L.bp_key(n, 4) for n in range(9)] == [(n // 4) << 17 | (n % 4) for n in range(9)]
    assert L.bp_key((1 << 17) * 3 + 5, 1 << 17) == (3 << 17) | 5
    assert [L.bp_keeps(n, 2, 0) for n in range(4)] == [1, 0, 1, 0] and [L.bp_keeps(n, 2, 1) for n in range(4)] == [0, 1, 0, 1]
    assert L.bp_keeps(7, 1, 0) == 1 and L.bp_keeps(7, 0, 0) == 1
    # genome/genome.go:1427-1444: the oracle carries the same table
    tab = (C.c_uint8 * 256).in_dll(O.lib(), "lmo_base2bit")
    assert [L.bp_base_code(c) for c in range(256)] == list(tab)
    for ln in (31, 32, 33, 35, 36, 200, 6000, 120_000, (1 << 28) - 1):
        nb = (ln + 3) // 4
        assert L.bp_slot_bytes(ln) % 8 == 0 and 16 <= L.bp_slot_bytes(ln) - nb <= 23


def test_new_declarations_are_exported_and_the_header_is_c99():
    import lexicmap_amd as la
    la.build_library()
    hdr = os.path.join(ROOT, "include", "lexicmap_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    declared = set(re.findall(r"\b(lm_[a-z0-9_]+)\s*\(", txt))
    assert all(s in declared for s in NEW_SYMBOLS)
    assert "lm_build_opt" in txt and "lm_contig" in txt
    out = subprocess.check_output(["nm", "-D", "--defined-only", la.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not [s for s in NEW_SYMBOLS if s not in exported]
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the Python view of lm_build_opt has the header's layout and the defaults of `lexicmap index`
    o = la.BuildOpt.default()
    assert (o.k, o.masks, o.mask_seed, o.max_desert, o.seed_dist, o.contig_interval, o.genome_batch_size, o.max_genome) == \
        (31, 20000, 1, 100, 50, 1000, 5000, 20_000_000)
    assert C.sizeof(la.BuildOpt) == 40
