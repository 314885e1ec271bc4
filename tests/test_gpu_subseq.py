"""Subject subsequences and flanks from a resident index on the GPU (lm_index_subseqs, lm_index_subseq_rows,
lm_index_genome_seqs, lm_format_subseqs; lexicmap_amd/csrc/lm_subseq.hip) against the plain model of tests/subseq_model.py, on
the fixture set of tests/genome_build_fixture.py (8 genomes, 9 records, G6 split), and against the reference's golden rows of
the two demo genomes.  Expected values come from the model, never from the library."""
import os
import random
import threading

import pytest

import genome_build_fixture as F
import oracle as O
import subseq_model as SM

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "demo")


def _la():
    import lexicmap_amd as la
    return la


def _bo(**kw):
    return _la().BuildOpt.default(max_genome=F.MAX_GENOME, **kw)


@pytest.fixture(scope="module")
def fx():
    la = _la()
    gs = F.genomes()
    gi = la.Index.from_genomes(gs, _bo(), options=la.api.default_options(output_seq=1))
    yield dict(gs=gs, gi=gi, m=SM.Model(gs), queries=F.queries(gs), d={cid: s for _, contigs in gs for cid, s in contigs})
    gi.close()


def _same(sub, exp, what=""):
    """a Subseqs against the model's answers: every field, the bases, the layout of the blob"""
    assert sub.n == len(exp), what
    seqs = sub.seqs
    end = 0
    for i, (d, e) in enumerate(zip(sub.info, exp)):
        assert d["status"] == e["status"], (what, i, d, e["status"])
        assert d["off"] % 16 == 0 and d["off"] >= end, (what, i)
        assert sub.blob[end:d["off"]] == bytes(d["off"] - end), (what, i)           # zeros between two regions
        end = d["off"] + d["len"]
        assert (d["begin"], d["end"], d["rc"]) == (e["begin"], e["end"], e["rc"]), (what, i, d, e["begin"], e["end"])
        if e["status"] != SM.OK:
            assert d["len"] == 0, (what, i)
            continue
        assert (d["key"], d["seq_idx"], d["len"]) == (e["key"], e["seq_idx"], len(e["seq"])), (what, i, d)
        assert seqs[i] == e["seq"], (what, i, d, seqs[i][:40], e["seq"][:40])
        assert d["genome_id"] == e["genome_id"].encode() and d["seq_id"] == (e["seq_id"].encode() if e["seq_id"] else None), (what, i, d)
    assert sub.blob[end:] == bytes(len(sub.blob) - end) and len(sub.blob) % 16 == 0


def _check(ix, m, regions, up=0, down=0, what=""):
    sub = ix.subseq(regions, up, down)
    _same(sub, m.run(regions, up, down), what)
    return sub


LENGTHS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def test_edges_of_the_kernel(fx):
    gi, m = fx["gi"], fx["m"]
    regions = []
    for ln in LENGTHS:
        for phase in range(4):
            for rc in (0, 1):
                b = 5000 + 4 * ln + phase                                            # begin % 4 = 0 .. 3
                regions.append(dict(key=0, seq_idx=0, begin=b, end=b + ln - 1, rc=rc))
                regions.append(dict(key=1, seq_id="G2_c", begin=40 + phase, end=39 + phase + ln, rc=rc))   # contig offset 62 025: another byte phase
    regions += [dict(key=3, seq_idx=0, begin=1, end=6000, rc=rc) for rc in (0, 1)]            # a whole contig
    regions += [dict(key=0, seq_idx=0, begin=1, end=120_000, rc=1)]
    regions += [dict(key=1, seq_idx=1, begin=26, end=30, rc=rc) for rc in (0, 1)]             # clamped away: no bases
    regions += [dict(key=8, seq_idx=0, begin=b, end=b + 3, rc=b & 1) for b in (201, 202, 205, 10 ** 9)]   # ... behind the LAST contig of the store
    regions += [dict(key=1, seq_idx=3, begin=40_002, end=40_002), dict(genome_id="G6", seq_id="G6_z", begin=30_007, end=30_010)]   # ... of a record
    regions += [dict(key=0, seq_idx=0, begin=1, end=1, rc=rc) for rc in (0, 1)]               # first base of the first record
    regions += [dict(key=8, seq_idx=0, begin=200, end=200, rc=rc) for rc in (0, 1)]           # last base of the last record: ends the store
    regions += [dict(key=8, seq_idx=0, begin=1, end=200), dict(key=8, begin=185, end=200, rc=1)]
    regions += [dict(key=1, begin=59_991, end=60_010, rc=rc) for rc in (0, 1)]                # concatenated, across a spacer: A's
    regions += [dict(key=1, begin=60_990, end=61_030), dict(key=1, begin=1, end=10 ** 9)]     # ... across G2_b; clamped to the record
    regions += [dict(key=2, seq_idx=0, begin=1, end=40), dict(key=2, seq_idx=0, begin=995, end=1010, rc=1),
                dict(key=2, seq_idx=0, begin=29_990, end=30_310), dict(key=2, seq_idx=0, begin=89_980, end=90_000, rc=1),
                dict(key=2, seq_idx=0, begin=29_495, end=29_545), dict(key=2, seq_idx=0, begin=30_899, end=30_905)]   # G3: N runs, lower case, YKR
    sub = _check(gi, m, regions, what="edges")
    exp = m.run(regions)
    assert exp[-1]["seq"][2:5] == b"CGA" and exp[-6]["seq"][:7] == b"AAAAAAA"                # (Y, K, R -> C, G, A; N -> A)
    assert sub.stats["pieces"] == 1 and sub.stats["answered"] == len(regions)
    assert sum(1 for d in sub.info if d["status"] == SM.OK and d["len"] == 0) == 8
    assert gi.subseq([dict(key=8, seq_idx=0, begin=202, end=205)]).info[0]["status"] == SM.OK      # no refusal without ignore_errors either
    # the text of a result that holds answered regions without bases: the header and an empty line (util.go:311-347)
    text = _la().format_subseqs(sub, line_width=60)
    assert text == SM.fasta(exp, 60) and text.count(b">G2_b:26-25:+\n\n") == 1 and text.count(b">G2_b:26-25:-\n\n") == 1
    assert _la().format_subseqs(sub, line_width=0) == SM.fasta(exp, 0)
    # flanks: the 25-b contig with 1000 on both sides is clamped to 25; a region ending with its contig gains nothing downstream
    flanked = [dict(key=1, seq_idx=1, begin=10, end=12, rc=rc) for rc in (0, 1)] + \
              [dict(key=1, seq_idx=0, begin=59_950, end=60_000), dict(key=1, seq_idx=0, begin=1, end=50, rc=1),
               dict(key=8, seq_idx=0, begin=150, end=200), dict(key=0, seq_idx=0, begin=3, end=5)]
    s2 = _check(gi, m, flanked, 1000, 1000, what="flanks 1000")
    assert [d["len"] for d in s2.info[:2]] == [25, 25] and (s2.info[0]["begin"], s2.info[0]["end"]) == (1, 25)
    s3 = _check(gi, m, flanked, 7, 50, what="flanks 7/50")
    assert (s3.info[2]["begin"], s3.info[2]["end"], s3.info[2]["len"]) == (59_943, 60_000, 58)
    assert (s3.info[3]["begin"], s3.info[3]["end"]) == (1, 57)                                  # '-': the flanks swap


def test_by_number_by_id_by_genome_and_genome_seqs(fx):
    gi, m, d = fx["gi"], fx["m"], fx["d"]
    regions = [dict(key=1, seq_idx=3, begin=101, end=1600), dict(key=1, seq_id="G2_d", begin=101, end=1600),
               dict(genome_id="G2", seq_id="G2_d", begin=101, end=1600, rc=1), dict(genome_id="G6", seq_id="G6_y", begin=1001, end=3000),
               dict(genome_id="G6", seq_id="G6_z", begin=29_990, end=30_000), dict(genome_id="G6", seq_id="G6_x", begin=1, end=20),
               dict(genome_id="G6", begin=99_990, end=100_010), dict(genome_id="G6", seq_idx=0, begin=5, end=9),
               dict(genome_id="G8", seq_id="G8_c", begin=1, end=200)]
    sub = _check(gi, m, regions, what="naming")
    assert sub.seqs[0] == sub.seqs[1] == d["G2_d"][100:1600] and sub.seqs[2] == SM.revcomp(d["G2_d"][100:1600])
    assert sub.info[3]["key"] == 6 and sub.seqs[3] == d["G6_y"][1000:3000]                     # the second record of the split genome
    assert sub.info[6]["key"] == 5 and sub.info[6]["seq_idx"] == -1 and sub.info[6]["end"] == 100_000   # concatenated: the first record
    la = _la()
    text = la.format_subseqs(sub, line_width=60)
    assert text == SM.fasta(m.run(regions), 60) and text.startswith(b">G2_d:101-1600:+\n") and b"\n>G6:99990-100000:+\n" in text
    assert la.format_subseqs(sub, line_width=0) == SM.fasta(m.run(regions), 0)
    g6 = gi.genome_seqs("G6")
    exp = m.genome_seqs("G6")
    assert [(x["seq_id"].decode(), s) for x, s in zip(g6.info, g6.seqs)] == exp and [c for c, _ in exp] == ["G6_x", "G6_y", "G6_z"]
    assert [x["key"] for x in g6.info] == [5, 6, 6] and [x["seq_idx"] for x in g6.info] == [0, 0, 1]
    ans = [dict(status=0, seq_idx=0, seq_id=c, genome_id="G6", begin=1, end=len(s), rc=0, seq=s) for c, s in exp]
    assert la.format_subseqs(g6, line_width=70) == SM.fasta(ans, 70, genome_seqs=True)
    g2 = gi.genome_seqs("G2")
    assert [len(s) for s in g2.seqs] == [60_000, 25, 1_200, 40_000]
    with pytest.raises(ValueError, match="reference name not found: G9"):
        gi.genome_seqs("G9")


def test_every_status_and_every_refusal(fx):
    gi, m = fx["gi"], fx["m"]
    bad = [(dict(key=99, seq_idx=0, begin=1, end=5), SM.NO_GENOME), (dict(genome_id="G9", seq_id="G9_c", begin=1, end=5), SM.NO_GENOME),
           (dict(key=1, seq_id="G2_e", begin=1, end=5), SM.NO_SEQ), (dict(key=1, seq_idx=4, begin=1, end=5), SM.NO_SEQ),
           (dict(genome_id="G6", seq_id="G1_c", begin=1, end=5), SM.NO_SEQ), (dict(genome_id="G6", seq_idx=1, begin=1, end=5), SM.NO_SEQ),
           (dict(key=8, begin=201, end=205), SM.OUT_OF_RANGE), (dict(key=5, begin=100_001, end=100_001, rc=1), SM.OUT_OF_RANGE)]
    good = dict(key=4, seq_idx=0, begin=11, end=30)
    regions = [good] + [r for r, _ in bad] + [good]
    sub = gi.subseq(regions, ignore_errors=True)
    _same(sub, m.run(regions), "statuses")
    assert [d["status"] for d in sub.info] == [0] + [s for _, s in bad] + [0] and sub.stats["answered"] == 2
    assert _la().format_subseqs(sub) == SM.fasta(m.run(regions), 60) and _la().format_subseqs(sub).count(b">") == 2
    for i, (r, st) in enumerate(bad):                                                   # without ignore_errors: the refusal
        with pytest.raises(ValueError, match="region 1 ") as e:
            gi.subseq([good, r, good])
        assert ("another shard" not in str(e.value)) and ("lm_index_subseqs" in str(e.value)), i
    with pytest.raises(ValueError, match="region 2: both begin and end"):
        gi.subseq([good, good, dict(key=4, seq_idx=0, begin=0, end=3)], ignore_errors=True)
    with pytest.raises(ValueError, match="region 0: begin position"):
        gi.subseq([dict(key=4, seq_idx=0, begin=5, end=4)])
    for up, down in ((-1, 0), (0, -1)):
        with pytest.raises(ValueError, match="upstream and downstream"):
            gi.subseq([good], up, down, ignore_errors=True)
    assert gi.subseq([]).n == 0 and gi.subseq([]).blob == b""
    _check(gi, m, [good], what="the handle is as good as new")


def _random_regions(m, seed, n):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        rec = rng.randrange(len(m.records))
        ci = rng.randrange(len(m.ids[rec]))
        size = m.sizes[rec][ci]
        b = rng.randrange(1, size + 1)
        e = b + rng.choice([0, 2, 15, 16, 40, 99, 300, 1000, 2500]) - rng.choice([0, 0, 1])
        r = dict(begin=b, end=max(b, e), rc=rng.randrange(2))
        how = rng.randrange(4)
        if how == 0:
            r.update(key=m.keys[rec], seq_idx=ci)
        elif how == 1:
            r.update(key=m.keys[rec], seq_id=m.ids[rec][ci])
        elif how == 2:
            r.update(genome_id=m.records[rec][0], seq_id=m.ids[rec][ci])
        else:
            r.update(key=m.keys[rec])                                                   # concatenated coordinates
        out.append(r)
    return out


def test_pieces_give_the_same_bytes(fx, monkeypatch):
    gi, m = fx["gi"], fx["m"]
    regions = _random_regions(m, 11, 2000) + [dict(key=0, seq_idx=0, begin=1, end=120_000), dict(key=6, begin=1, end=10 ** 6, rc=1)]
    monkeypatch.delenv("LM_SUBSEQ_PIECE_BYTES", raising=False)
    one = gi.subseq(regions, 9, 33)
    _same(one, m.run(regions, 9, 33), "one piece")
    monkeypatch.setenv("LM_SUBSEQ_PIECE_BYTES", "4096")
    many = gi.subseq(regions, 9, 33)
    assert one.stats["pieces"] == 1 and many.stats["pieces"] == (len(one.blob) + 4095) // 4096 > 100
    assert many.blob == one.blob and many.info == one.info
    monkeypatch.setenv("LM_SUBSEQ_PIECE_BYTES", "48")                                     # three lanes per piece, an odd number of pieces
    few = regions[:40]
    a = gi.subseq(few)
    monkeypatch.delenv("LM_SUBSEQ_PIECE_BYTES")
    b = gi.subseq(few)
    assert a.blob == b.blob and a.stats["pieces"] == (len(b.blob) + 47) // 48 and b.stats["pieces"] == 1


def test_every_kind_of_handle_gives_the_same_bytes(fx, tmp_path):
    la = _la()
    gi, m, gs = fx["gi"], fx["m"], fx["gs"]
    regions = _random_regions(m, 23, 300) + [dict(key=8, seq_idx=0, begin=190, end=200), dict(key=0, seq_idx=0, begin=1, end=17, rc=1)]
    exp = m.run(regions, 5, 40)
    want = gi.subseq(regions, 5, 40)
    _same(want, exp, "built")
    host = la.api.Residency(la.api.GENOMES_HOST)
    small = la.Index.from_genomes(gs, _bo(masks=1024))
    handles = []
    try:
        gi.save(str(tmp_path / "saved.lmi"), 2)
        handles.append(("opened", la.Index(str(tmp_path / "saved.lmi"))))
        part = la.Index.from_genomes(gs[:5], _bo(masks=1024))
        rest = la.Index.from_genomes(gs[5:], _bo(masks=1024))
        handles += [("part", part), ("rest", rest)]
        handles.append(("extended", part.extend(gs[5:], _bo(masks=1024))))                 # (G6 needs max_genome)
        handles.append(("joined", part.join(rest)))
        handles.append(("host", la.Index.from_genomes(gs, _bo(masks=1024), residency=host)))
        handles.append(("opened on the host", la.Index(str(tmp_path / "saved.lmi"), residency=host)))
        full_bytes = handles[0][1].residency()["genome_bytes_device"]
        auto = la.Index(str(tmp_path / "saved.lmi"), residency=la.api.Residency(la.api.GENOMES_AUTO, full_bytes // 2))
        handles.append(("split by AUTO", auto))
        r = auto.residency()
        assert r["genomes_device"] > 0 and r["genomes_host"] > 0, r
        for name, ix in handles:
            if name in ("part", "rest"):
                continue
            got = ix.subseq(regions, 5, 40)
            _same(got, exp, name)
            assert got.blob == want.blob, name
        # a subset: records 0, 2, 5, 6, 8 become 0 .. 4 (keys remapped)
        sub = small.subset([8, 2, 6, 0, 5])
        handles.append(("subset", sub))
        d = dict(gs)
        ms = SM.Model([(n, d[n]) for n in ("G1", "G3", "G6", "G8")])
        sregions = _random_regions(ms, 29, 200) + [dict(genome_id="G6", seq_id="G6_z", begin=1, end=30_000, rc=1)]
        _check(sub, ms, sregions, 5, 40, what="subset")
        assert sub.subseq([dict(key=5, seq_idx=0, begin=1, end=2)], ignore_errors=True).info[0]["status"] == SM.NO_GENOME
    finally:
        small.close()
        for _, ix in handles:
            ix.close()


def test_three_shards_answer_for_their_own_records(fx):
    la = _la()
    gi, m, gs = fx["gi"], fx["m"], fx["gs"]
    regions = [dict(key=k, seq_idx=0, begin=10, end=400, rc=k & 1) for k in range(9)] + _random_regions(m, 31, 300)
    want = gi.subseq(regions, 3, 3)
    shards = [la.Index.from_genomes(gs, _bo(masks=1024), options=la.api.default_options(shard_rank=r, shard_count=3)) for r in range(3)]
    try:
        answers = [s.subseq(regions, 3, 3, ignore_errors=True) for s in shards]
        local = [{i for i in range(9) if a.info[i]["status"] == SM.OK} for a in answers]
        assert sorted(x for l in local for x in l) == list(range(9)) and all(local)       # every record on exactly one shard
        assert any({5, 6} <= l for l in local)                                             # the split genome stays together
        for r, a in enumerate(answers):
            _same(a, m.run(regions, 3, 3, local=local[r]), "shard %d" % r)
            assert {d["status"] for d in a.info} == {SM.OK, SM.NOT_LOCAL, SM.NO_GENOME}       # (by name: the shard's own genomes only)
        for i in range(len(regions)):                                                     # the union is the unsharded answer
            ok = [a for a in answers if a.info[i]["status"] == SM.OK]
            assert len(ok) == 1 and ok[0].seqs[i] == want.seqs[i], i
        other = next(k for k in range(9) if k not in local[0])
        with pytest.raises(ValueError, match="region 0 .*another shard"):
            shards[0].subseq([dict(key=other, seq_idx=0, begin=1, end=5)])
    finally:
        for s in shards:
            s.close()


def test_a_sharded_synthetic_handle_tells_another_shards_record_from_no_record():
    """a synthetic set has no tables of the other shards' records: a key is another shard's when it is a genome number of the set"""
    la = _la()
    kw = dict(genomes=6, genome_len=20_000, families=2, seed=77, masks=1024)
    whole = la.Index.synthetic(**kw)
    shards = [la.Index.synthetic(options=la.api.default_options(shard_rank=r, shard_count=2), **kw) for r in range(2)]
    try:
        nowhere = [6, 5000, 1 << 17, (1 << 17) | 3]                                       # behind the set; no such index in a batch; no such batch
        regions = [dict(key=k, seq_idx=0, begin=101 + k % 6, end=1100, rc=k & 1) for k in list(range(6)) + nowhere]
        want = whole.subseq(regions, 5, 5, ignore_errors=True)
        assert [d["status"] for d in want.info] == [SM.OK] * 6 + [SM.NO_GENOME] * 4 and all(len(s) == 1010 - k for k, s in enumerate(want.seqs[:6]))
        answers = [s.subseq(regions, 5, 5, ignore_errors=True) for s in shards]
        for a in answers:
            assert {d["status"] for d in a.info[:6]} == {SM.OK, SM.NOT_LOCAL} and [d["status"] for d in a.info[6:]] == [SM.NO_GENOME] * 4
        for i in range(6):                                                                # the union is the unsharded answer
            ok = [a for a in answers if a.info[i]["status"] == SM.OK]
            assert len(ok) == 1 and ok[0].seqs[i] == want.seqs[i], i
        with pytest.raises(ValueError, match="region 0 ") as e:
            shards[0].subseq([dict(key=6, seq_idx=0, begin=1, end=5)])
        assert "another shard" not in str(e.value) and "not in this index" in str(e.value)
    finally:
        whole.close()
        for s in shards:
            s.close()


def _gapless(rows, i):
    return _la().api.row_strings(rows, i)[2].replace("-", "").encode()


def test_rows_of_a_search(fx):
    la = _la()
    gi, m, gs = fx["gi"], fx["m"], fx["gs"]
    qb = gi.upload(fx["queries"])
    rows, _ = gi.search_resident_np(qb)
    gi.free_batch(qb)
    assert len(rows) >= 7 and {int(k) for k in rows["batch_genome"]} >= {0, 1, 2, 3, 4, 6, 7} and set(rows["rc"]) <= {0, 1}
    sub = gi.subseq_rows(rows)
    regions = [m.row_region(r) for r in rows]
    _same(sub, m.run(regions), "rows")
    for i in range(len(rows)):                                                            # the row's own -a column, gaps removed
        assert sub.seqs[i] == _gapless(rows, i), i
    _same(gi.subseq_rows(rows, 7, 1300), m.run(regions, 7, 1300), "rows with flanks")
    as_dicts, _ = gi.search(fx["queries"])                                                # the list-of-dicts form of the same rows
    assert gi.subseq_rows(as_dicts, 7, 1300).blob == gi.subseq_rows(rows, 7, 1300).blob
    # The rows of two shards, merged in one process.  Two ranks cannot share one device, so the wire of lm_gather_merge_rows is
    # not crossed here (tests/test_gpu_gather_two_procs.py does that): the rows pass through its two merges instead - the host
    # merge lm_merge_sharded with the names re-attached, and below the device merge that lm_gather_merge_rows runs behind the
    # gather, on rows whose pointer columns are cleared as the gather clears them.  The regions are the unsharded ones.
    tb = gi.info()["total_bases"]
    shards = [la.Index.from_genomes(gs, _bo(), options=la.api.default_options(shard_rank=r, shard_count=2, total_bases_override=tb))
              for r in range(2)]
    try:
        per = []
        for s in shards:
            q = s.upload(fx["queries"])
            per.append(s.search_resident_np(q)[0])
            s.free_batch(q)
        from lexicmap_amd import merge
        merged, _names = merge.merge_sharded_c(per, index=shards[0])
        assert len(merged) > 0 and (merged["genome_id"] == 0).all()
        mregions = [m.row_region(r) for r in merged]
        assert {r["key"] for r in mregions} == {r["key"] for r in regions}
        _same(gi.subseq_rows(merged, 7, 1300), m.run(mregions, 7, 1300), "merged rows")
        parts = [s.subseq_rows(merged, 7, 1300, ignore_errors=True) for s in shards]
        exp = m.run(mregions, 7, 1300)
        for i in range(len(merged)):
            ok = [p for p in parts if p.info[i]["status"] == SM.OK]
            assert len(ok) == 1 and ok[0].seqs[i] == exp[i]["seq"], i
        import numpy as np
        import torch
        cat = merge._cat(per)
        for f in merge.PTR_FIELDS:
            cat[f] = 0
        dev = torch.from_numpy(cat.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        comm = la.api.Comm(la.api.Comm.unique_id(), 1, 0, device=0)
        try:
            dmerged = comm.merge_sharded_device(dev.data_ptr(), [len(p) for p in per]).copy()
        finally:
            comm.close()
        assert len(dmerged) == len(merged) and (dmerged["genome_id"] == 0).all() and (dmerged["seq_id"] == 0).all()
        dregions = [m.row_region(r) for r in dmerged]
        assert sorted((r["key"], r["begin"], r["end"]) for r in dregions) == sorted((r["key"], r["begin"], r["end"]) for r in mregions)
        _same(gi.subseq_rows(dmerged, 7, 1300), m.run(dregions, 7, 1300), "rows of the device merge")
    finally:
        for s in shards:
            s.close()


def test_reference_golden_rows_and_the_fasta_text(tmp_path):
    """the two demo genomes, -a -n 2 as test_gpu_parity does: the bases of every row against the reference's own sseq column"""
    la = _la()
    d = str(tmp_path / "demo2.lmi")
    genomes = [(f[:-6], O.read_fasta(os.path.join(GOLD, f))) for f in ("GCF_002949675.1.fa.gz", "GCF_003697165.2.fa.gz")]
    O.build_index(d, genomes, O.default_build_opt(chunks=4))
    q = O.read_fasta(os.path.join(GOLD, "q.gene.fasta"))[0]
    gold = [l.split("\t") for l in open(os.path.join(GOLD, "q.gene.fasta.lexicmap_top-2-genomes_all.tsv")).read().rstrip("\n").split("\n")[1:]]
    gi = la.Index(d, la.api.default_options(top_n_genomes=2, output_seq=1))
    try:
        qb = gi.upload([q[1]])
        rows, _ = gi.search_resident_np(qb)
        gi.free_batch(qb)
        assert len(rows) == len(gold) == 14
        sub = gi.subseq_rows(rows)
        for i, c in enumerate(gold):
            assert sub.seqs[i].decode() == c[22].replace("-", ""), i
            assert (sub.info[i]["begin"], sub.info[i]["end"], "-" if sub.info[i]["rc"] else "+") == (int(c[14]), int(c[15]), c[16])
            assert (sub.info[i]["genome_id"].decode(), sub.info[i]["seq_id"].decode()) == (c[3], c[4])
        # utils subseq -U 20 -D 30: the text, with the long header made of the row's own TSV columns
        m = SM.Model(records=genomes)
        flank = gi.subseq_rows(rows, 20, 30)
        regions = [dict(genome_id=c[3], seq_id=c[4], begin=int(c[14]), end=int(c[15]), rc=c[16] == "-") for c in gold]
        exp = m.run(regions, 20, 30)
        tsv = ["\t".join(c[:20]) for c in gold]
        text = la.format_subseqs(flank, rows, [q[0]], [len(q[1])], line_width=60)
        assert text == SM.fasta(exp, 60, tsv=tsv)
        assert text.startswith(b">NZ_CP033092.2:458539-460130:+ query=NC_000913.3:4166659-4168200 sgenome=GCF_003697165.2 ")
        assert la.format_subseqs(flank, line_width=60) == SM.fasta(exp, 60)
    finally:
        gi.close()


def test_a_search_on_another_thread_returns_its_usual_rows(fx):
    gi, m = fx["gi"], fx["m"]
    base, _ = gi.search(fx["queries"])
    regions = _random_regions(m, 41, 500)
    exp = m.run(regions, 10, 10)
    out = {}

    def searcher():
        out["rows"] = [gi.search(fx["queries"])[0] for _ in range(2)]
    t = threading.Thread(target=searcher)
    t.start()
    subs = [gi.subseq(regions, 10, 10) for _ in range(3)]
    t.join()
    assert out["rows"] == [base, base]
    for s in subs:
        _same(s, exp, "beside a search")
