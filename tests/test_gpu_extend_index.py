"""Genomes added to a resident index (lm_index_builder_extend, Index.extend): the extended index against ONE build of all the
genomes with the same masks - info(), mask lists, genome bytes, rows, saved files - and the rows against the oracle's.
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


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """base, extended and one-shot index with 20 000 and with 1024 masks (the build with thousands of desert seeds), once"""
    la = _la()
    gs = F.genomes()
    A, B = gs[:5], gs[5:]
    out = dict(gs=gs, A=A, B=B, queries=F.queries(gs), tmp=tmp_path_factory.mktemp("extend"))
    opened = []
    for tag, M in (("", 20000), ("2", 1024)):
        base = la.Index.from_genomes(A, _bo(masks=M))
        base_rows = _rows(base, out["queries"])
        ext = base.extend(B, _bo(masks=M))
        full = la.Index.from_genomes(gs, _bo(masks=M))
        opened += [base, ext, full]
        out.update({"base" + tag: base, "ext" + tag: ext, "full" + tag: full, "base_rows" + tag: base_rows})
    out["full_lists2"] = _lists(out["full2"], range(1024))
    out["full_lists"] = _lists(out["full"], _sample(20000))
    out["full_rows"] = _rows(out["full"], out["queries"])
    yield out
    for ix in opened:
        ix.close()


def test_extended_index_equals_the_one_shot_build(fx):
    ext, full = fx["ext"], fx["full"]
    assert fx["base"].info()["genomes"] == 5 and ext.info()["genomes"] == 9
    _same_info(ext.info(), full.info())
    _same_info(fx["ext2"].info(), fx["full2"].info())
    _same_lists(_lists(ext, _sample(20000)), fx["full_lists"])
    _same_lists(_lists(fx["ext2"], range(1024)), fx["full_lists2"])
    # (the 1024-mask lists hold desert seeds of base AND added records: more than one k-mer of a genome under a mask)
    keys = set()
    for kv in fx["full_lists2"].values():
        per = {}
        for k, v in kv:
            if not v & 1:
                per.setdefault(v >> 30, set()).add(k)
        keys |= {g for g, s in per.items() if len(s) > 1}
    assert keys & {0, 1, 2, 4} and keys & {5, 6, 7}
    recs = F.records(fx["gs"])
    assert _fetch_all(ext, recs) == _fetch_all(full, recs) == [F.concatenation(c) for _, c in recs]
    rows = _rows(ext, fx["queries"])
    assert rows == fx["full_rows"]
    assert {r["batch_genome"] for r in rows[0]} == {0, 7}            # a base genome and an added one under one query
    assert rows[2][0]["batch_genome"] == 6 and rows[2][0]["nchunks"] == 2 and rows[2][0]["chunk_idx"] == 1   # the added chunk list
    d = str(fx["tmp"] / "oracle_all.lmi")
    O.build_index(d, fx["gs"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=_masks(fx["base"]))
    _assert_oracle_rows(rows, d, fx["queries"])


def test_saved_files_are_byte_identical(fx):
    da, db = str(fx["tmp"] / "ext.lmi"), str(fx["tmp"] / "full.lmi")
    fx["ext"].save(da, chunks=4)
    fx["full"].save(db, chunks=4)
    names = []
    for root, _, files in os.walk(da):
        names += [os.path.relpath(os.path.join(root, f), da) for f in files]
    other = []
    for root, _, files in os.walk(db):
        other += [os.path.relpath(os.path.join(root, f), db) for f in files]
    assert sorted(names) == sorted(other) and "genomes.chunks.bin" in names and len(names) > 12
    _, mismatch, errors = filecmp.cmpfiles(da, db, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def test_value_widths_grow_and_the_base_is_only_read(fx):
    la = _la()
    d = dict(fx["gs"])
    base_gs = [("G8", d["G8"]), ("G4", d["G4"])]
    add_gs = [("G1", d["G1"]), ("G3", d["G3"]), ("G6", d["G6"])]
    qs = [fx["queries"][3], fx["queries"][0], fx["queries"][2]]          # G4 (base), G1, G6_y (added)
    base = la.Index.from_genomes(base_gs, _bo())
    try:
        before = _rows(base, qs)
        assert len(before[0]) > 0
        ext = base.extend(add_gs, _bo())
        full = la.Index.from_genomes(base_gs + add_gs, _bo())
        try:
            assert ext.info()["val_bits"] > base.info()["val_bits"]      # 1 + 13 + 1 bits -> 3 + 17 + 1
            _same_info(ext.info(), full.info())
            _same_lists(_lists(ext, _sample(20000)), _lists(full, _sample(20000)))
            rows = _rows(ext, qs)
            assert rows == _rows(full, qs) and all(len(r) > 0 for r in rows)
            assert _rows(base, qs) == before                                # searched again after finish()
            assert base.info()["genomes"] == 2
        finally:
            ext.close()
            full.close()
    finally:
        base.close()


def test_batch_boundary_and_extending_twice(fx):
    la = _la()
    d = dict(fx["gs"])
    base = la.Index.from_genomes(fx["A"], _bo(genome_batch_size=4))       # records 0..4: batch 1 holds one
    e1 = base.extend([("G6", d["G6"])], _bo(genome_batch_size=4))         # 5, 6: inside batch 1
    e2 = e1.extend([("G7", d["G7"]), ("G8", d["G8"])])                   # 7 fills batch 1, 8 opens batch 2; settings from the handle
    full = la.Index.from_genomes(fx["gs"], _bo(genome_batch_size=4))
    try:
        _same_info(e2.info(), full.info())
        got = _lists(e2, _sample(20000))
        _same_lists(got, _lists(full, _sample(20000)))
        assert {v >> 30 for kv in got.values() for _, v in kv} == {(n // 4) << 17 | (n % 4) for n in range(9)}
        rows = _rows(e2, fx["queries"])
        assert rows == _rows(full, fx["queries"])
        assert rows[2][0]["batch_genome"] == (1 << 17) | 2
    finally:
        for ix in (base, e1, e2, full):
            ix.close()


def test_extending_an_index_opened_from_disk(fx):
    la = _la()
    tmp = fx["tmp"]
    # (a) saved by this library with settings away from the defaults: the extend takes them from info.toml
    bo = dict(masks=1024, max_desert=150, seed_dist=60)
    built = la.Index.from_genomes(fx["A"], _bo(**bo))
    d = str(tmp / "a150.lmi")
    built.save(d, chunks=2)
    built.close()
    base = la.Index(d)
    ext = base.extend(fx["B"], la.BuildOpt.default(masks=1024, max_desert=150, seed_dist=60, max_genome=F.MAX_GENOME))
    ext0 = base.extend([(g, c) for g, c in fx["B"] if g != "G6"])          # no build options at all (G6 needs max_genome)
    full = la.Index.from_genomes(fx["gs"], _bo(**bo))
    full0 = la.Index.from_genomes([(g, c) for g, c in fx["gs"] if g != "G6"], _bo(**bo))
    dflt = la.Index.from_genomes(fx["gs"], _bo(masks=1024))
    try:
        _same_info(ext.info(), full.info())
        _same_lists(_lists(ext, range(1024)), _lists(full, range(1024)))
        _same_info(ext0.info(), full0.info())
        _same_lists(_lists(ext0, range(1024)), _lists(full0, range(1024)))   # deserts filled with 150 / 60, read from the file
        assert full.info()["seeds"] != dflt.info()["seeds"]                   # (the settings matter for this set)
        assert _rows(ext, fx["queries"]) == _rows(full, fx["queries"])
        s = str(tmp / "a150ext.lmi")
        ext.save(s, chunks=2)
        info = open(os.path.join(s, "info.toml")).read()
        assert "max-seed-dist = 150\n" in info and "seed-dist-in-desert = 60\n" in info and "input-genomes = 8\n" in info
    finally:
        for ix in (base, ext, ext0, full, full0, dflt):
            ix.close()
    # (b) written by the oracle's writer
    masks = _masks(fx["base"])
    da, dall = str(tmp / "oracle_a.lmi"), str(tmp / "oracle_all2.lmi")
    O.build_index(da, fx["A"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=masks)
    O.build_index(dall, fx["gs"], O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=masks)
    oa, oall = la.Index(da), la.Index(dall)
    ext = oa.extend(fx["B"], _bo())
    try:
        a, b = ext.info(), oall.info()
        for f in ("seeds", "genomes", "genome_bases", "total_bases", "outlier_seeds", "key_bits", "val_bits"):
            assert a[f] == b[f], (f, a[f], b[f])
        _same_lists(_lists(ext, _sample(20000)), _lists(oall, _sample(20000)))
        assert _rows(ext, fx["queries"]) == _rows(oall, fx["queries"])
        recs = F.records(fx["gs"])
        assert _fetch_all(ext, recs) == _fetch_all(oall, recs)
    finally:
        for ix in (oa, oall, ext):
            ix.close()


def test_base_seeds_decoded_in_many_pieces(fx, monkeypatch, capfd):
    """staging pieces far smaller than the base's image, and smaller than its largest list: many pieces, lists cut"""
    base = fx["base2"]
    longest = max(max(len(base.mask_seeds(m)[0]) for m in range(1024)), 8)
    piece = max(4, longest // 3)
    nseeds = base.info()["seeds"]
    assert nseeds > 50 * piece
    monkeypatch.setenv("LM_BUILD_STAGE_SEEDS", str(piece))
    monkeypatch.setenv("LM_DEBUG", "1")
    capfd.readouterr()
    ext = base.extend(fx["B"], _bo(masks=1024))
    try:
        assert "decoded and packed in pieces of %d:" % piece in capfd.readouterr().err
        _same_info(ext.info(), fx["full2"].info())
        _same_lists(_lists(ext, range(1024)), fx["full_lists2"])
    finally:
        ext.close()


@pytest.mark.parametrize("rank", [0, 1])
def test_shards(fx, rank):
    la = _la()
    opt = la.api.default_options(shard_rank=rank, shard_count=2)
    base = la.Index.from_genomes(fx["A"], _bo(), options=opt)
    ext = base.extend(fx["B"], _bo())
    full = la.Index.from_genomes(fx["gs"], _bo(), options=la.api.default_options(shard_rank=rank, shard_count=2))
    try:
        _same_info(ext.info(), full.info())
        got = _lists(ext, _sample(20000))
        _same_lists(got, _lists(full, _sample(20000)))
        assert {v >> 30 for kv in got.values() for _, v in kv} == ({0, 2, 4, 8}, {1, 3, 5, 6, 7})[rank]
        assert _rows(ext, fx["queries"]) == _rows(full, fx["queries"])
    finally:
        for ix in (base, ext, full):
            ix.close()


def test_host_resident_genomes(fx):
    la = _la()
    host = la.api.Residency(la.api.GENOMES_HOST)
    base = la.Index.from_genomes(fx["A"], _bo(), residency=host)
    ext = base.extend(fx["B"], _bo(), residency=la.api.Residency(la.api.GENOMES_HOST))
    try:
        assert base.residency()["genomes_host"] == 5
        r = ext.residency()
        assert r["genomes_device"] == 0 and r["genomes_host"] == 9
        assert _rows(ext, fx["queries"]) == fx["full_rows"]
        recs = F.records(fx["gs"])
        assert _fetch_all(ext, recs) == [F.concatenation(c) for _, c in recs]
    finally:
        base.close()
        ext.close()


def test_errors(fx, tmp_path):
    la = _la()
    L = la.lib()
    base = fx["base"]
    for field, kw in (("masks", dict(masks=1024)), ("k", dict(k=21)), ("contig_interval", dict(contig_interval=500)),
                      ("genome_batch_size", dict(genome_batch_size=4))):
        with pytest.raises(RuntimeError) as ei:
            la.IndexBuilder.extending(base, _bo(**kw))
        assert ei.value.status == 7 and field in str(ei.value), (field, str(ei.value))
    # a refused genome leaves the builder usable
    b = la.IndexBuilder.extending(base, _bo())
    try:
        for i, (gid, contigs) in enumerate(fx["B"]):
            if i == 1:
                assert b.try_add("big", [("ok", b"ACGT" * 100), ("b", b"ACGT" * 40_000)]) == 7 and "big genome" in b.last_error()
                assert b.try_add("tiny", [("t", b"ACGTA")]) == 7 and "shorter than k" in b.last_error()
            b.add(gid, contigs)
        ext = b.finish()
    finally:
        b.close()
    try:
        _same_info(ext.info(), fx["full"].info())
        _same_lists(_lists(ext, _sample(20000)), fx["full_lists"])
        assert _rows(ext, fx["queries"]) == fx["full_rows"]
    finally:
        ext.close()
    # nothing added
    b = la.IndexBuilder.extending(base)
    h = C.c_void_p()
    assert L.lm_index_builder_finish(b.h, C.byref(h)) == 7 and not h
    b.h = None
    assert b"no genome" in L.lm_last_error(None)
    assert _rows(base, fx["queries"][:1]) == fx["base_rows"][:1]             # and the base is as it was
    # irregular batches: 5 records saved in batches of 4 (4 + 1), opened as if the batch size were 3
    b4 = la.Index.from_genomes(fx["A"], _bo(genome_batch_size=4))
    d = str(tmp_path / "b4.lmi")
    b4.save(d, chunks=2)
    b4.close()
    p = os.path.join(d, "info.toml")
    txt = open(p).read()
    assert "genome-batch-size = 4\n" in txt
    open(p, "w").write(txt.replace("genome-batch-size = 4\n", "genome-batch-size = 3\n"))
    li = la.Index(d)
    try:
        with pytest.raises(RuntimeError) as ei:
            la.IndexBuilder.extending(li)
        assert ei.value.status == 7 and "irregular" in str(ei.value)
    finally:
        li.close()
