"""Resident indexes joined and subset through the index builder (lm_index_builder_add_index / _like, Index.join / subset,
IndexBuilder.add_index / like): the result against ONE build of the same genomes in the same order with the same masks -
info(), mask lists, genome bytes, rows, saved files - and the rows against the oracle's.
Fixture set: tests/genome_build_fixture.py; A = G1..G5 (5 records), B = G6 (split into two records), G7 (a mutated G1), G8."""
import ctypes as C
import filecmp
import os

import pytest

import genome_build_fixture as F
import oracle as O

pytestmark = pytest.mark.gpu

ROW_FIELDS = ("batch_genome", "aligned_length", "qbegin", "qend", "tbegin", "tend", "bitscore", "gaps", "pident",
              "seq_idx", "nchunks", "chunk_idx", "genome_id", "seq_id")
MORE_FIELDS = ("hits", "hsp", "cls", "evalue", "score")


def _la():
    import lexicmap_amd as la
    return la


def _bo(**kw):
    return _la().BuildOpt.default(max_genome=F.MAX_GENOME, **kw)


def _masks(gi):
    p = _la().lib().lm_index_masks(gi.h)
    return [p[i] for i in range(gi.info()["masks"])]


def _lists(ix, sample):
    out = {}
    for m in sample:
        k, v = ix.mask_seeds(m)
        out[m] = sorted(zip(k.tolist(), v.tolist()))
    return out


def _same_lists(a, b):
    assert a.keys() == b.keys()
    for m in a:
        assert a[m] == b[m], (m, len(a[m]), len(b[m]), [x for x in a[m] if x not in b[m]][:3], [x for x in b[m] if x not in a[m]][:3])


def _rows(ix, queries, fields=ROW_FIELDS + MORE_FIELDS):
    rows, _ = ix.search(queries)
    return [[{f: r[f] for f in fields} for r in rows if r["query"] == qi] for qi in range(len(queries))]


def _same_info(a, b):
    """every field of lm_index_info, the byte counts among them: the same arrays of the same sizes"""
    for f in a:
        assert a[f] == b[f], (f, a[f], b[f])


def _assert_oracle_rows(got, d, queries):
    oi = O.Index(d)
    try:
        for qi, q in enumerate(queries):
            exp = oi.search(q)[0]
            assert len(exp) > 0 and len(exp) == len(got[qi]), (qi, len(exp), len(got[qi]))
            for g, e in zip(got[qi], exp):
                for f in ROW_FIELDS + ("hsp", "cls", "score"):
                    assert g[f] == e[f], (qi, f, g[f], e[f])
                assert g["evalue"] == pytest.approx(e["evalue"], rel=1e-9, abs=0)
    finally:
        oi.close()


def _sample(M):
    return list(range(0, M, 7)) + [M - 1]


def _fetch_all(ix, recs):
    return [ix.fetch(l, 0, len(F.concatenation(c))) for l, (_, c) in enumerate(recs)]


def _keys(lists):
    return {v >> 30 for kv in lists.values() for _, v in kv}


def _same_saved_trees(a, b, da, db, chunks=4):
    a.save(da, chunks=chunks)
    b.save(db, chunks=chunks)
    names, other = [], []
    for root, _, files in os.walk(da):
        names += [os.path.relpath(os.path.join(root, f), da) for f in files]
    for root, _, files in os.walk(db):
        other += [os.path.relpath(os.path.join(root, f), db) for f in files]
    assert sorted(names) == sorted(other) and "genomes.chunks.bin" in names and len(names) >= 8
    _, mismatch, errors = filecmp.cmpfiles(da, db, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def _same_index(got, full, queries, recs, sample, full_lists=None, full_rows=None):
    """info, lists, fetched bases of every record, rows; returns (lists, rows) of `got`"""
    _same_info(got.info(), full.info())
    lists = _lists(got, sample)
    _same_lists(lists, full_lists if full_lists is not None else _lists(full, sample))
    assert _fetch_all(got, recs) == _fetch_all(full, recs) == [F.concatenation(c) for _, c in recs]
    rows = _rows(got, queries)
    assert rows == (full_rows if full_rows is not None else _rows(full, queries))
    return lists, rows


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """the two parts, their join and the one-shot index with 20 000 and with 1024 masks (the build with thousands of desert
    seeds), once"""
    la = _la()
    gs = F.genomes()
    A, B = gs[:5], gs[5:]
    out = dict(gs=gs, A=A, B=B, queries=F.queries(gs), recs=F.records(gs), tmp=tmp_path_factory.mktemp("join"))
    opened = []
    for tag, M in (("", 20000), ("2", 1024)):
        a = la.Index.from_genomes(A, _bo(masks=M))
        b = la.Index.from_genomes(B, _bo(masks=M))
        rows_ab = (_rows(a, out["queries"]), _rows(b, out["queries"]))
        joined = a.join(b)
        full = la.Index.from_genomes(gs, _bo(masks=M))
        opened += [a, b, joined, full]
        out.update({"a" + tag: a, "b" + tag: b, "join" + tag: joined, "full" + tag: full, "rows_ab" + tag: rows_ab})
    out["full_lists2"] = _lists(out["full2"], range(1024))
    out["full_lists"] = _lists(out["full"], _sample(20000))
    out["full_rows"] = _rows(out["full"], out["queries"])
    out["full_rows2"] = _rows(out["full2"], out["queries"])
    yield out
    for ix in opened:
        ix.close()


# ---- 1. join equals one build
@pytest.mark.parametrize("tag,M", [("", 20000), ("2", 1024)])
def test_join_equals_the_one_shot_build(fx, tag, M):
    a, b, joined, full = fx["a" + tag], fx["b" + tag], fx["join" + tag], fx["full" + tag]
    assert a.info()["genomes"] == 5 and b.info()["genomes"] == 4 and joined.info()["genomes"] == 9
    sample = _sample(M) if M == 20000 else range(M)
    lists, rows = _same_index(joined, full, fx["queries"], fx["recs"], sample, fx["full_lists" + tag], fx["full_rows" + tag])
    assert _keys(lists) == set(range(9))
    assert {r["batch_genome"] for r in rows[0]} == {0, 7}            # a genome of A and one of B under one query
    assert rows[2][0]["batch_genome"] == 6 and rows[2][0]["nchunks"] == 2 and rows[2][0]["chunk_idx"] == 1   # B's chunk list
    if M == 1024:
        # desert seeds of both sides were carried: more than one k-mer of a genome under a mask
        multi = set()
        for kv in lists.values():
            per = {}
            for k, v in kv:
                if not v & 1:
                    per.setdefault(v >> 30, set()).add(k)
            multi |= {g for g, s in per.items() if len(s) > 1}
        assert multi & {0, 1, 2, 4} and multi & {5, 6, 7}
    d = str(fx["tmp"] / ("oracle_all%s.lmi" % tag))
    O.build_index(d, fx["gs"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME, masks=M), masks=_masks(a))
    _assert_oracle_rows(rows, d, fx["queries"])
    _same_saved_trees(joined, full, str(fx["tmp"] / ("join%s.lmi" % tag)), str(fx["tmp"] / ("full%s.lmi" % tag)))
    # the parts are as they were
    assert (_rows(a, fx["queries"]), _rows(b, fx["queries"])) == fx["rows_ab" + tag]


# ---- 2. both parts hold a split genome
def test_two_chunk_lists(fx):
    la = _la()
    d = dict(fx["gs"])
    # a second split genome from fixture contigs under new names: [H_p], [H_q + spacer + H_r]
    H = ("H", [("H_p", d["G1"][0][1]), ("H_q", d["G2"][0][1]), ("H_r", d["G3"][0][1])])
    part1 = [("G5", d["G5"]), ("G6", d["G6"]), ("G4", d["G4"])]
    part2 = [("G8", d["G8"]), H, ("G7", d["G7"])]
    recs = F.records(part1 + part2)
    assert len(recs) == 8 and [g for g, _ in recs].count("H") == 2
    hrec = max(i for i, (g, _) in enumerate(recs) if g == "H")
    qs = [fx["queries"][2], d["G3"][0][1][50_000:51_500], fx["queries"][3]]   # G6_y (part 1's list), H_r (part 2's), G4
    p1, p2 = la.Index.from_genomes(part1, _bo(masks=1024)), la.Index.from_genomes(part2, _bo(masks=1024))
    joined = p1.join(p2)
    full = la.Index.from_genomes(part1 + part2, _bo(masks=1024))
    try:
        _, rows = _same_index(joined, full, qs, recs, range(1024))
        assert rows[0][0]["batch_genome"] == 2 and rows[0][0]["nchunks"] == 2 and rows[0][0]["chunk_idx"] == 1
        assert rows[1][0]["batch_genome"] == hrec and rows[1][0]["nchunks"] == 2 and rows[1][0]["chunk_idx"] == 1
        assert rows[1][0]["genome_id"] == b"H" and rows[1][0]["seq_id"] == b"H_r"
        _same_saved_trees(joined, full, str(fx["tmp"] / "two_lists_join.lmi"), str(fx["tmp"] / "two_lists_full.lmi"), chunks=2)
        assert os.path.getsize(str(fx["tmp"] / "two_lists_join.lmi" / "genomes.chunks.bin")) == 2 * (8 + 2 * 8)
    finally:
        for ix in (p1, p2, joined, full):
            ix.close()


# ---- 3. value widths grow, the inputs are only read
def test_value_widths_grow_and_the_inputs_are_only_read(fx):
    la = _la()
    d = dict(fx["gs"])
    base_gs = [("G8", d["G8"]), ("G4", d["G4"])]
    part_gs = [("G1", d["G1"]), ("G3", d["G3"]), ("G6", d["G6"])]
    qs = [fx["queries"][3], fx["queries"][0], fx["queries"][2]]          # G4 (base), G1, G6_y (part)
    base, part = la.Index.from_genomes(base_gs, _bo()), la.Index.from_genomes(part_gs, _bo())
    try:
        before = (_rows(base, qs), _rows(part, qs))
        assert len(before[0][0]) > 0 and len(before[1][1]) > 0
        joined = base.join(part)
        full = la.Index.from_genomes(base_gs + part_gs, _bo())
        try:
            assert joined.info()["val_bits"] > part.info()["val_bits"] > base.info()["val_bits"]   # 3 + 17 + 1 > 2 + 17 + 1 > 1 + 13 + 1
            _, rows = _same_index(joined, full, qs, F.records(base_gs + part_gs), _sample(20000))
            assert all(len(r) > 0 for r in rows)
            assert (_rows(base, qs), _rows(part, qs)) == before            # searched again after finish()
            assert base.info()["genomes"] == 2 and part.info()["genomes"] == 4
        finally:
            joined.close()
            full.close()
    finally:
        base.close()
        part.close()


# ---- 4. add and add_index interleaved, several sources
@pytest.mark.parametrize("batch", [5000, 4])
def test_interleaving_and_n_way(fx, batch):
    la = _la()
    d = dict(fx["gs"])
    g = lambda n: (n, d[n])
    order = [g("G1"), g("G2"), g("G3"), g("G4"), g("G5"), g("G6"), g("G8")]
    s1 = la.Index.from_genomes([g("G2"), g("G3")], _bo(masks=1024))
    s2 = la.Index.from_genomes([g("G5"), g("G6")], _bo(masks=1024))
    full = la.Index.from_genomes(order, _bo(masks=1024, genome_batch_size=batch))
    b = la.IndexBuilder(_bo(masks=1024, genome_batch_size=batch))
    try:
        b.add(*g("G1"))
        b.add_index(s1)
        b.add(*g("G4"))
        b.add_index(s2)
        b.add(*g("G8"))
        got = b.finish()
    finally:
        b.close()
    try:
        qs = fx["queries"][1:]                                           # (G7 is not in this set: query 0 would differ from the fixture's rows)
        lists, rows = _same_index(got, full, qs, F.records(order), range(1024))
        assert _keys(lists) == {(n // batch) << 17 | (n % batch) for n in range(8)}
        assert rows[1][0]["batch_genome"] == ((6 // batch) << 17 | 6 % batch) and rows[1][0]["nchunks"] == 2   # G6_y: record 6
        _same_saved_trees(got, full, str(fx["tmp"] / ("inter%d.lmi" % batch)), str(fx["tmp"] / ("inter%d_full.lmi" % batch)), chunks=2)
    finally:
        for ix in (s1, s2, full, got):
            ix.close()


# ---- 5. subset
SUBSET_RECORDS = (0, 2, 5, 6, 8)     # G1, G3, G6 (both records), G8


@pytest.fixture(scope="module")
def subref(fx):
    """one build of the kept genomes with 1024 masks, and all of its lists"""
    d = dict(fx["gs"])
    gs = [(n, d[n]) for n in ("G1", "G3", "G6", "G8")]
    ref = _la().Index.from_genomes(gs, _bo(masks=1024))
    yield dict(gs=gs, ref=ref, lists=_lists(ref, range(1024)))
    ref.close()


def test_subset_equals_the_one_shot_build(fx, subref):
    full2 = fx["full2"]
    sub = full2.subset([8, 2, 6, 0, 5])
    try:
        qs = [fx["queries"][0], fx["queries"][1], fx["queries"][2]]
        lists, rows = _same_index(sub, subref["ref"], qs, F.records(subref["gs"]), range(1024), subref["lists"])
        assert _keys(lists) == set(range(5))                             # no value carries an old key (7 or 8 would be one)
        assert {r["batch_genome"] for r in rows[0]} == {0}               # G7 is gone
        assert rows[2][0]["batch_genome"] == 3 and rows[2][0]["nchunks"] == 2 and rows[2][0]["chunk_idx"] == 1
        _same_saved_trees(sub, subref["ref"], str(fx["tmp"] / "sub.lmi"), str(fx["tmp"] / "sub_ref.lmi"), chunks=2)
        assert _rows(full2, fx["queries"]) == fx["full_rows2"]          # the source is as it was
    finally:
        sub.close()


def test_subset_decoded_in_many_pieces(fx, subref, monkeypatch, capfd):
    """staging pieces far smaller than the source's image, and smaller than its largest list: many pieces, lists cut"""
    full2 = fx["full2"]
    longest = max(max(len(v) for v in fx["full_lists2"].values()), 8)
    piece = max(4, longest // 3)
    assert full2.info()["seeds"] > 50 * piece
    monkeypatch.setenv("LM_BUILD_STAGE_SEEDS", str(piece))
    monkeypatch.setenv("LM_DEBUG", "1")
    capfd.readouterr()
    sub = full2.subset([SUBSET_RECORDS[i] for i in (3, 1, 4, 0, 2)])
    try:
        err = capfd.readouterr().err
        assert "keys rewritten, compacted) decoded and packed in pieces of %d:" % piece in err
        _same_info(sub.info(), subref["ref"].info())
        _same_lists(_lists(sub, range(1024)), subref["lists"])
    finally:
        sub.close()


def test_subset_of_one_tiny_genome(fx):
    """G8 alone (200 bases, record 8): nearly every decode piece comes out empty"""
    la = _la()
    d = dict(fx["gs"])
    sub = fx["full2"].subset([8])
    ref = la.Index.from_genomes([("G8", d["G8"])], _bo(masks=1024))
    try:
        q = [d["G8"][0][1]]
        lists, rows = _same_index(sub, ref, q, F.records([("G8", d["G8"])]), range(1024))
        assert _keys(lists) == {0} and sub.info()["genomes"] == 1
    finally:
        sub.close()
        ref.close()


# ---- 6. sources from disk and from the host
def test_sources_from_disk_and_from_the_host(fx):
    la = _la()
    tmp = fx["tmp"]
    a, b = fx["a"], fx["b"]
    recs = fx["recs"]
    # (a) a source saved by this library and opened again
    db = str(tmp / "b_saved.lmi")
    b.save(db, chunks=2)
    ob = la.Index(db)
    j = a.join(ob)
    try:
        _same_index(j, fx["full"], fx["queries"], recs, _sample(20000), fx["full_lists"], fx["full_rows"])
    finally:
        j.close()
        ob.close()
    # (b) written by the oracle's writer
    masks = _masks(a)
    da, dbb, dall = str(tmp / "oracle_a.lmi"), str(tmp / "oracle_b.lmi"), str(tmp / "oracle_all.lmi")
    O.build_index(da, fx["A"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=masks)
    O.build_index(dbb, fx["B"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=masks)
    if not os.path.isdir(dall):                                           # (the join test of 20 000 masks writes it too)
        O.build_index(dall, fx["gs"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=masks)
    oa, ob, oall = la.Index(da), la.Index(dbb), la.Index(dall)
    j = oa.join(ob)
    try:
        x, y = j.info(), oall.info()
        for f in ("seeds", "genomes", "genome_bases", "total_bases", "outlier_seeds", "key_bits", "val_bits"):
            assert x[f] == y[f], (f, x[f], y[f])
        _same_lists(_lists(j, _sample(20000)), _lists(oall, _sample(20000)))
        assert _rows(j, fx["queries"]) == _rows(oall, fx["queries"]) == fx["full_rows"]
        assert _fetch_all(j, recs) == _fetch_all(oall, recs)
    finally:
        for ix in (oa, ob, oall, j):
            ix.close()
    # (c) a source whose genomes live in pinned host memory, and (d) a result asked for there
    host = la.api.Residency(la.api.GENOMES_HOST)
    hb = la.Index.from_genomes(fx["B"], _bo(), residency=host)
    j = a.join(hb)
    jh = a.join(hb, residency=la.api.Residency(la.api.GENOMES_HOST))
    try:
        assert hb.residency()["genomes_host"] == 4 and hb.residency()["genomes_device"] == 0
        assert j.residency()["genomes_device"] == 9 and j.residency()["genomes_host"] == 0
        _same_index(j, fx["full"], fx["queries"], recs, _sample(20000), fx["full_lists"], fx["full_rows"])
        r = jh.residency()
        assert r["genomes_device"] == 0 and r["genomes_host"] == 9
        assert _fetch_all(jh, recs) == [F.concatenation(c) for _, c in recs]
        assert _rows(jh, fx["queries"]) == fx["full_rows"]
    finally:
        for ix in (hb, j, jh):
            ix.close()


# ---- 7. a source with irregular batches
def test_irregular_source(fx):
    """5 records saved in batches of 4 (4 + 1), opened as if the batch size were 3: refused as a base, a legal source"""
    la = _la()
    b4 = la.Index.from_genomes(fx["A"], _bo(genome_batch_size=4))
    d = str(fx["tmp"] / "b4.lmi")
    b4.save(d, chunks=2)
    b4.close()
    p = os.path.join(d, "info.toml")
    txt = open(p).read()
    assert "genome-batch-size = 4\n" in txt
    open(p, "w").write(txt.replace("genome-batch-size = 4\n", "genome-batch-size = 3\n"))
    li = la.Index(d)
    ref = la.Index.from_genomes(fx["A"], _bo(genome_batch_size=3))
    try:
        with pytest.raises(RuntimeError) as ei:
            la.IndexBuilder.extending(li)
        assert ei.value.status == 7 and "irregular" in str(ei.value)
        b = la.IndexBuilder.like(li)
        try:
            got = b.add_index(li).finish()
        finally:
            b.close()
        try:
            lists, _ = _same_index(got, ref, fx["queries"][1:2] + fx["queries"][3:], F.records(fx["A"]), _sample(20000))
            assert _keys(lists) == {(n // 3) << 17 | n % 3 for n in range(5)}
            assert got.info()["genomes"] == 5
        finally:
            got.close()
    finally:
        li.close()
        ref.close()


# ---- 8. refusals
def test_errors(fx):
    la = _la()
    L = la.lib()
    a, b = fx["a"], fx["b"]
    sharded = la.api.default_options(shard_rank=0, shard_count=2)
    other_seed = la.Index.from_genomes(fx["B"][2:], _bo(mask_seed=2))
    other_ci = la.Index.from_genomes(fx["B"][2:], _bo(contig_interval=500))
    shard = la.Index.from_genomes(fx["B"], _bo(), options=sharded)
    dk = str(fx["tmp"] / "k21.lmi")
    O.build_index(dk, fx["A"][3:4], O.default_build_opt(chunks=2, k=21))
    other_k = la.Index(dk)
    bkeys = [0, 1, 2, 3]                                                   # B alone: G6 = 0, 1 (one split genome), G7 = 2, G8 = 3
    bld = la.IndexBuilder.extending(a, _bo())
    try:
        def refused(src, keep, *words):
            assert bld.try_add_index(src, keep) == 7
            txt = bld.last_error()
            for w in words:
                assert w in txt, (w, txt)
            with pytest.raises(ValueError):
                bld.add_index(src, keep)
        refused(other_seed, None, "mask values differ")
        refused(other_k, None, "k differs", "21")
        refused(other_ci, None, "contig_interval differs", "500")
        refused(shard, None, "shard 0 of 2")
        refused(a, None, "the index this builder continues")
        refused(b, bkeys + [9], "no record of the source")
        refused(b, [2, 3, 2], "twice")
        refused(b, [1, 2, 3], "1 of the 2 records of a split genome")
        refused(b, [], "empty")
        bld.add_index(b, [3, 2, 1, 0])                                     # every record, named one by one
        refused(b, None, "added to the builder before")
        got = bld.finish()
    finally:
        bld.close()
    try:
        _same_index(got, fx["full"], fx["queries"], fx["recs"], _sample(20000), fx["full_lists"], fx["full_rows"])
    finally:
        got.close()
    # a sharded builder takes no source
    sb = la.IndexBuilder(_bo(), options=sharded)
    try:
        assert sb.try_add_index(b) == 7 and "the builder is sharded" in sb.last_error()
    finally:
        sb.close()
    # like() with options that disagree is refused as extending() is
    for field, kw in (("masks", dict(masks=1024)), ("k", dict(k=21)), ("contig_interval", dict(contig_interval=500)),
                      ("genome_batch_size", dict(genome_batch_size=4))):
        with pytest.raises(RuntimeError) as ei:
            la.IndexBuilder.like(a, _bo(**kw))
        assert ei.value.status == 7 and field in str(ei.value) and "lm_index_builder_like" in str(ei.value), (field, str(ei.value))
    # finish after only refused calls
    nb = la.IndexBuilder.like(a)
    assert nb.try_add_index(other_seed) == 7 and nb.try_add_index(b, []) == 7
    h = C.c_void_p()
    assert L.lm_index_builder_finish(nb.h, C.byref(h)) == 7 and not h
    nb.h = None
    assert b"no genome" in L.lm_last_error(None)
    assert (_rows(a, fx["queries"]), _rows(b, fx["queries"])) == fx["rows_ab"]   # and the sources are as they were
    for ix in (other_seed, other_ci, shard, other_k):
        ix.close()
