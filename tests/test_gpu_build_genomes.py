"""Index built on the GPU from caller-supplied genomes (lm_index_builder_*, Index.from_genomes): every mask list, the genome
bytes, the rows, the saved files, the keys, the shards and the residency of the result against the oracle's index writer
(oracle/lmo_build.c) run on the same genomes with the same masks.  Fixture set: tests/genome_build_fixture.py."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import genome_build_fixture as F
import oracle as O

pytestmark = pytest.mark.gpu

ROW_FIELDS = ("batch_genome", "aligned_length", "qbegin", "qend", "tbegin", "tend", "bitscore", "gaps", "pident",
              "seq_idx", "nchunks", "chunk_idx", "genome_id", "seq_id")


def _masks(gi):
    import lexicmap_amd as la
    M = gi.info()["masks"]
    p = la.lib().lm_index_masks(gi.h)
    return [p[i] for i in range(M)]


def _lists(ix, sample):
    out = {}
    for m in sample:
        k, v = ix.mask_seeds(m)
        out[m] = sorted(zip(k.tolist(), v.tolist()))
    return out


def _same_lists(a, b):
    for m in a:
        assert a[m] == b[m], (m, len(a[m]), len(b[m]), [x for x in a[m] if x not in b[m]][:3], [x for x in b[m] if x not in a[m]][:3])


def _rows(ix, queries):
    rows, _ = ix.search(queries)
    return [[{f: r[f] for f in ROW_FIELDS} for r in rows if r["query"] == qi] for qi in range(len(queries))]


def _oracle_rows(d, queries):
    oi = O.Index(d)
    out = [[{f: r[f] for f in ROW_FIELDS} for r in oi.search(q)[0]] for q in queries]
    oi.close()
    return out


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """the fixture set built once by the GPU builder and once by the oracle's writer (same masks), and what both give"""
    import lexicmap_amd as la
    gs = F.genomes()
    gi = la.Index.from_genomes(gs, la.BuildOpt.default(max_genome=F.MAX_GENOME))
    masks = _masks(gi)
    M = len(masks)
    d = str(tmp_path_factory.mktemp("build") / "oracle.lmi")
    O.build_index(d, gs, O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=masks)
    oi = la.Index(d)
    sample = list(range(0, M, 7)) + [M - 1]
    qs = F.queries(gs)
    # The same set with 1024 masks.  With 20 000 masks a genome of 6 .. 120 kb has a seed every 3 .. 6 bases: a gap of 100 has
    # the probability e^-17 and the oracle writer's index of this set holds NO desert seed at all (counted: 0).  1024 masks put G1's 1024 captures
    # 117 bases apart on average, e^(-100/117) = 43 % of the gaps are deserts and
    # the oracle's index holds 9 222 desert seeds, next to every spacer, N run and low-complexity stretch of the set.
    gi2 = la.Index.from_genomes(gs, la.BuildOpt.default(max_genome=F.MAX_GENOME, masks=1024))
    masks2 = _masks(gi2)
    d2 = str(tmp_path_factory.mktemp("build") / "oracle1024.lmi")
    O.build_index(d2, gs, O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME, masks=1024), masks=masks2)
    oi2 = la.Index(d2)
    out = dict(gs=gs, gi=gi, oi=oi, dir=d, masks=masks, M=M, sample=sample, queries=qs,
               oracle_rows=_oracle_rows(d, qs), gpu_lists=_lists(gi, sample), gi2=gi2, oi2=oi2, dir2=d2)
    yield out
    for ix in (gi, oi, gi2, oi2):
        ix.close()


def test_every_mask_list_equals_the_oracle_writers(fx):
    """captures with skip regions and the missing-prefix rule, desert filling with intervals, reversed seeds: the (k-mer,
    value) lists under the sampled masks are the oracle writer's, and the hard parts were among what was compared.
    Compared: the sampled masks of the build with the default 20 000 masks (the missing-prefix rule: G4, G8) and ALL lists of
    the build of the same genomes with 1024 masks (desert seeds: the fixture comment says why 20 000 masks leave none)."""
    gi, oi = fx["gi"], fx["oi"]
    a, b = gi.info(), oi.info()
    for f in ("seeds", "genomes", "genome_bases", "total_bases"):
        assert a[f] == b[f], (f, a[f], b[f])
    assert a["genomes"] == 9
    got = fx["gpu_lists"]
    _same_lists(got, _lists(oi, fx["sample"]))
    a2, b2 = fx["gi2"].info(), fx["oi2"].info()
    for f in ("seeds", "genomes", "genome_bases", "total_bases"):
        assert a2[f] == b2[f], (f, a2[f], b2[f])
    got2 = _lists(fx["gi2"], range(1024))
    _same_lists(got2, _lists(fx["oi2"], range(1024)))
    keys, g3_pos, desert = set(), [], 0
    for m, kv in list(got.items()) + list(got2.items()):
        per_genome = {}
        for k, v in kv:
            key = v >> 30
            keys.add(key)
            if key == 2:
                g3_pos.append((v >> 2) & ((1 << 28) - 1))
            if not v & 1:
                per_genome.setdefault(key, set()).add(k)
        desert += sum(1 for s in per_genome.values() if len(s) > 1)
    assert keys == set(range(9))                    # G4 (3) and both records of G6 (5, 6) among them
    # (mask, genome) pairs with more than one k-mer = desert seeds.  G1 alone: ~0.43 x 1024 gaps of >= 100 bases, each filled
    # every 50 bases under one of 1024 masks - more than a tenth of the masks must hold one
    assert desert > 100
    assert g3_pos and not [p for p in g3_pos if 30_000 - 30 <= p <= 30_299]   # nothing of G3 overlaps its 300 N
    assert all(any((v >> 30) == 2 and not v & 1 for _, v in kv) for kv in got2.values())   # (G3 was inside the 1024-mask lists)
    # G4 has 6 kb: 2 x 5970 k-mers meet 4^7 prefixes, so most masks take the missing-prefix rule - and every sampled mask
    # holds a normal seed of G4 or dropped a low-complexity capture
    n4 = sum(1 for kv in got.values() if any((v >> 30) == 3 and not v & 1 for _, v in kv))
    assert n4 > 0.9 * len(got)


def test_genome_bytes_are_the_two_bit_round_trip_of_the_concatenation(fx):
    recs = F.records(fx["gs"])
    assert len(recs) == 9
    for l, (gid, contigs) in enumerate(recs):
        exp = F.concatenation(contigs)
        assert fx["gi"].fetch(l, 0, len(exp)) == exp, (l, gid)
    g3 = fx["gi"].fetch(2, 0, 90_000)
    assert g3[:7] == b"A" * 7 and g3[1000:1004] == b"AAAA" and g3[30_900:30_903] == b"CGA" and g3[-9:] == b"A" * 9


def test_rows_equal_the_oracles(fx):
    got = _rows(fx["gi"], fx["queries"])
    exp = fx["oracle_rows"]
    for qi, (g, e) in enumerate(zip(got, exp)):
        assert len(e) > 0 and g == e, (qi, g[:2], e[:2])
    assert {r["batch_genome"] for r in got[0]} == {0, 7}                                   # G1 and its 5 % sibling
    assert got[2][0]["batch_genome"] == 6 and got[2][0]["nchunks"] == 2 and got[2][0]["chunk_idx"] == 1
    assert got[2][0]["genome_id"] == b"G6" and got[2][0]["seq_id"] == b"G6_y"
    assert got[4][0]["seq_idx"] == 3 and got[4][0]["seq_id"] == b"G2_d"
    rows, _ = fx["gi"].search(fx["queries"])
    r = [x for x in rows if x["query"] == 4][0]
    assert (r["nseqs"], r["seq_len"]) == (4, 40_000)
    assert _rows(fx["oi"], fx["queries"]) == got      # and the loader's handle of the oracle-written index says the same


def test_save_and_reopen(fx, tmp_path):
    import lexicmap_amd as la
    d = str(tmp_path / "saved.lmi")
    fx["gi"].save(d, chunks=3)
    li = la.Index(d)
    a, b = fx["gi"].info(), li.info()
    for f in ("k", "masks", "genomes", "seeds", "genome_bases", "total_bases", "outlier_seeds", "key_bits", "partition_bases"):
        assert a[f] == b[f], f
    _same_lists(fx["gpu_lists"], _lists(li, fx["sample"]))
    assert _rows(li, fx["queries"]) == fx["oracle_rows"]
    li.close()
    assert _oracle_rows(d, fx["queries"]) == fx["oracle_rows"]
    cb = open(os.path.join(d, "genomes.chunks.bin"), "rb").read()
    assert struct.unpack(">3Q", cb) == (2, 5, 6)
    info = open(os.path.join(d, "info.toml")).read()
    assert "input-genomes = 8\n" in info and "genomes = 9\n" in info and "genome-batch-size = 5000\n" in info


def test_genome_batch_size_4_gives_three_batches(fx, tmp_path):
    import lexicmap_amd as la
    gi = la.Index.from_genomes(fx["gs"], la.BuildOpt.default(max_genome=F.MAX_GENOME, genome_batch_size=4))
    try:
        d = str(tmp_path / "b4.lmi")
        O.build_index(d, fx["gs"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME, batch_size=4), masks=fx["masks"])
        assert sorted(os.listdir(os.path.join(d, "genomes"))) == ["batch_0000", "batch_0001", "batch_0002"]
        oi = la.Index(d)
        got = _lists(gi, fx["sample"])
        _same_lists(got, _lists(oi, fx["sample"]))
        oi.close()
        keys = {v >> 30 for kv in got.values() for _, v in kv}
        assert keys == {(n // 4) << 17 | (n % 4) for n in range(9)}
        rows = _rows(gi, fx["queries"])
        assert rows == _oracle_rows(d, fx["queries"])
        assert rows[2][0]["batch_genome"] == (1 << 17) | 2
        s = str(tmp_path / "b4saved.lmi")      # and lm_index_save keeps the batches
        gi.save(s, chunks=2)
        assert sorted(os.listdir(os.path.join(s, "genomes"))) == ["batch_0000", "batch_0001", "batch_0002"]
        assert _oracle_rows(s, fx["queries"]) == rows
    finally:
        gi.close()


def test_same_as_the_synthetic_builder_where_both_apply():
    """one contig, ACGT only, equal lengths: the new capture / desert kernels give the lists of the synthetic builder's"""
    import lexicmap_amd as la
    si = la.Index.synthetic(genomes=6, genome_len=200_000, families=2)
    try:
        gs = [("SYN_%09d.1" % g, [("syn%09d_c1" % g, si.fetch(g, 0, 200_000))]) for g in range(6)]
        gi = la.Index.from_genomes(gs)
        try:
            assert _masks(gi) == _masks(si)
            a, b = gi.info(), si.info()
            for f in ("seeds", "genomes", "genome_bases", "total_bases", "outlier_seeds"):
                assert a[f] == b[f], f
            M = a["masks"]
            sample = list(range(0, M, 7)) + [M - 1]
            _same_lists(_lists(gi, sample), _lists(si, sample))
        finally:
            gi.close()
    finally:
        si.close()


def test_shards_keep_what_the_loader_keeps(fx):
    import lexicmap_amd as la
    seen = []
    for rank in (0, 1):
        opt = la.api.default_options(shard_rank=rank, shard_count=2)
        gi = la.Index.from_genomes(fx["gs"], la.BuildOpt.default(max_genome=F.MAX_GENOME), options=opt)
        oi = la.Index(fx["dir"], options=la.api.default_options(shard_rank=rank, shard_count=2))
        try:
            a, b = gi.info(), oi.info()
            for f in ("seeds", "genomes", "genome_bases", "total_bases"):
                assert a[f] == b[f], (rank, f)
            got = _lists(gi, fx["sample"])
            _same_lists(got, _lists(oi, fx["sample"]))
            seen.append({v >> 30 for kv in got.values() for _, v in kv})
            rows, exp = _rows(gi, fx["queries"]), _rows(oi, fx["queries"])
            assert rows == exp
        finally:
            gi.close()
            oi.close()
    assert seen == [{0, 2, 4, 8}, {1, 3, 5, 6, 7}]      # both records of G6 with the rank of its first (5 % 2)


def test_host_resident_genomes_give_the_same_rows(fx):
    import lexicmap_amd as la
    gi = la.Index.from_genomes(fx["gs"], la.BuildOpt.default(max_genome=F.MAX_GENOME),
                               residency=la.api.Residency(la.api.GENOMES_HOST))
    try:
        r = gi.residency()
        assert r["genomes_device"] == 0 and r["genomes_host"] == 9
        assert _rows(gi, fx["queries"]) == fx["oracle_rows"]
        exp = F.concatenation(F.records(fx["gs"])[6][1])
        assert gi.fetch(6, 0, len(exp)) == exp
    finally:
        gi.close()


def test_refusals_leave_the_builder_usable(fx, monkeypatch):
    import lexicmap_amd as la
    L = la.lib()
    monkeypatch.setenv("LM_BUILD_SLAB_KB", "64")     # and the store grows through many small slabs meanwhile
    b = la.IndexBuilder(la.BuildOpt.default(max_genome=F.MAX_GENOME))
    try:
        gs = fx["gs"]
        for i, (gid, contigs) in enumerate(gs):
            if i == 2:
                assert b.try_add("tiny", [("t", b"ACGTA")]) == 7 and "shorter than k" in b.last_error()
            if i == 5:
                assert b.try_add("big", [("ok", b"ACGT" * 100), ("b", b"ACGT" * 40_000)]) == 7
                assert "big genome" in b.last_error()
                assert b.try_add("none", []) == 7 and b.last_error()
            b.add(gid, contigs)
        gi = b.finish()
    finally:
        b.close()
    try:
        a, e = gi.info(), fx["gi"].info()
        for f in ("seeds", "genomes", "genome_bases", "total_bases"):
            assert a[f] == e[f], f
        _same_lists(fx["gpu_lists"], _lists(gi, fx["sample"]))
        assert _rows(gi, fx["queries"]) == fx["oracle_rows"]
    finally:
        gi.close()
    monkeypatch.delenv("LM_BUILD_SLAB_KB")
    b = la.IndexBuilder()
    h = C.c_void_p()
    assert L.lm_index_builder_finish(b.h, C.byref(h)) == 7 and not h     # nothing added; the builder is consumed
    b.h = None
    assert b"no genome" in L.lm_last_error(None)
    with pytest.raises(RuntimeError) as ei:
        la.IndexBuilder(la.BuildOpt.default(k=21))
    assert ei.value.status == 7


def test_mask_count_beyond_the_lds_takes_the_global_minima_table(fx, tmp_path):
    """24 000 masks x 8 B do not fit the 160 KB of LDS of a CU: the capture keeps its per-mask minima in device memory
    (k_capture_g<false>).  Same set, same comparison: the sampled lists, info() and the rows against the oracle's writer."""
    import lexicmap_amd as la
    M = 24_000
    gi = la.Index.from_genomes(fx["gs"], la.BuildOpt.default(max_genome=F.MAX_GENOME, masks=M))
    try:
        masks = _masks(gi)
        assert len(masks) == M and M * 8 > 160 * 1024
        d = str(tmp_path / "m24000.lmi")
        O.build_index(d, fx["gs"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME, masks=M), masks=masks)
        oi = la.Index(d)
        try:
            a, b = gi.info(), oi.info()
            for f in ("seeds", "genomes", "genome_bases", "total_bases", "outlier_seeds"):
                assert a[f] == b[f], (f, a[f], b[f])
            sample = list(range(0, M, 7)) + [M - 1]
            got = _lists(gi, sample)
            _same_lists(got, _lists(oi, sample))
            assert {v >> 30 for kv in got.values() for _, v in kv} == set(range(9))
            # G4 and G8 under (nearly) every mask: the missing-prefix rule ran on the global table too
            for key in (3, 8):
                assert sum(1 for kv in got.values() if any((v >> 30) == key and not v & 1 for _, v in kv)) > 0.9 * len(got)
        finally:
            oi.close()
        assert _rows(gi, fx["queries"]) == _oracle_rows(d, fx["queries"])
    finally:
        gi.close()


@pytest.mark.parametrize("first", [4096, 12_000, 25_000])
def test_staging_arrays_that_overflow_are_enlarged_and_the_chunk_is_generated_again(fx, monkeypatch, capfd, first):
    """the 1024-mask build holds about 8 000 captures, as many desert seeds again, and a reversed twin of each: seed staging
    arrays of 4096 entries overflow in the capture, of 12 000 in the desert filling, of 25 000 in the reversed seeds - each is
    noticed from the counters (no store past an array), the arrays are cut again and the chunk regenerated to the same index"""
    import lexicmap_amd as la
    n = fx["gi2"].info()["seeds"]
    assert 25_000 < n < 2 * 25_000 and 12_000 < n // 2 < 25_000     # (the sizes above straddle what they are meant to)
    monkeypatch.setenv("LM_BUILD_STAGE_SEEDS", str(first))
    monkeypatch.setenv("LM_DEBUG", "1")
    capfd.readouterr()
    gi = la.Index.from_genomes(fx["gs"], la.BuildOpt.default(max_genome=F.MAX_GENOME, masks=1024))
    try:
        assert "staging buffers enlarged" in capfd.readouterr().err      # (the builder says so under LM_DEBUG)
        assert gi.info()["seeds"] == n
        _same_lists(_lists(fx["gi2"], range(1024)), _lists(gi, range(1024)))
    finally:
        gi.close()


def test_saved_info_carries_the_build_settings(tmp_path):
    import lexicmap_amd as la
    gs = F.genomes()[3:5]
    gi = la.Index.from_genomes(gs, la.BuildOpt.default(masks=1024, mask_seed=7, max_desert=150, seed_dist=60))
    try:
        d = str(tmp_path / "s.lmi")
        gi.save(d, chunks=2)
        info = open(os.path.join(d, "info.toml")).read()
        for line in ("masks = 1024", "rand-seed = 7", "max-seed-dist = 150", "seed-dist-in-desert = 60", "input-genomes = 2"):
            assert line + "\n" in info, line
        li = la.Index(d)
        assert li.info()["seeds"] == gi.info()["seeds"]
        li.close()
    finally:
        gi.close()
