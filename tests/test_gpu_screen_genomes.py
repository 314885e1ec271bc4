"""Genome screening on the GPU (lm_index_screen_genomes, Index.screen) against the Python model over the oracle
(tests/screen_model.py): every comparison is exact, row for row and field for field.  Index: the fixture set of
tests/genome_build_fixture.py, built once per module by Index.from_genomes and by the oracle's writer with the same masks."""
import ctypes as C
import os
import random

import pytest

import genome_build_fixture as F
import mask_sets as MS
import oracle as O
import screen_model as SM

pytestmark = pytest.mark.gpu

FIELDS = ("score", "batch_genome", "genome_id", "keys", "score2", "hit_masks", "hit_kmers", "prefixes")


def _norm(rows):
    out = []
    for qrows in rows:
        q = []
        for r in qrows:
            d = {f: r[f] for f in FIELDS}
            if isinstance(d["genome_id"], bytes):
                d["genome_id"] = d["genome_id"].decode()
            q.append(d)
        out.append(q)
    return out


def _same(got, exp):
    got, exp = _norm(got), _norm(exp)
    assert len(got) == len(exp)
    for qi, (g, e) in enumerate(zip(got, exp)):
        assert len(g) == len(e), (qi, [(r["batch_genome"], r["score"]) for r in g], [(r["batch_genome"], r["score"]) for r in e])
        for ri, (a, b) in enumerate(zip(g, e)):
            for f in FIELDS:
                assert a[f] == b[f], (qi, ri, f, a[f] if f != "prefixes" else a[f][:8], b[f] if f != "prefixes" else b[f][:8])


def _queries(gs):
    d = dict(gs)
    rng = random.Random(77)
    unrelated = bytes(rng.choice(b"ACGT") for _ in range(50_000))
    return [("G1", d["G1"]), ("G7", d["G7"]), ("G2", d["G2"]), ("G3", d["G3"]), ("G4", d["G4"]), ("G6", d["G6"]), ("G8", d["G8"]),
            ("short", [("short_c", d["G1"][0][1][:20])]), ("unrelated", [("u_c", unrelated)])]


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    import lexicmap_amd as la
    gs = F.genomes()
    gi = la.Index.from_genomes(gs, la.BuildOpt.default(max_genome=F.MAX_GENOME))
    masks = gi.masks().tolist()
    tmp = tmp_path_factory.mktemp("screen")
    d = str(tmp / "oracle.lmi")
    O.build_index(d, gs, O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=masks)
    recs = F.records(gs)
    names = {i: r[0] for i, r in enumerate(recs)}
    model = SM.Model(d, F.K, masks, SM.chunk_lists(recs), names)
    qs = _queries(gs)
    out = dict(la=la, gs=gs, gi=gi, dir=d, tmp=tmp, masks=masks, M=len(masks), model=model, qs=qs, recs=recs, names=names,
               exp=model.screen(qs, details=True, top_n=0))
    yield out
    model.close()
    gi.close()


def test_the_batch_equals_the_model_row_for_row(fx):
    got = fx["gi"].screen(fx["qs"], details=True, top_n=0)
    exp = fx["exp"]
    _same(got, exp)
    names = [q[0] for q in fx["qs"]]
    g = dict(zip(names, _norm(got)))
    # G1: itself first with the full length on every hit mask, its 5 % sibling second
    assert g["G1"][0]["batch_genome"] == 0 and set(g["G1"][0]["prefixes"]) == {F.K} and g["G1"][0]["hit_masks"] > 0.9 * fx["M"]
    assert g["G1"][1]["batch_genome"] == 7 and g["G7"][0]["batch_genome"] == 7 and g["G7"][1]["batch_genome"] == 0
    assert g["G2"][0]["batch_genome"] == 1 and g["G4"][0]["batch_genome"] == 3 and g["G8"][0]["batch_genome"] == 8
    # G3: its N runs are not skipped here; builder-style regions would give other rows
    assert g["G3"][0]["batch_genome"] == 2
    other = fx["model"].screen_one(dict(fx["gs"])["G3"], details=True, top_n=0, n_runs_skipped=True)
    assert _norm([other]) != _norm([exp[3]])
    # G6: both records hit, one row of two keys, the summed score, details of the lower key
    per = fx["model"].per_record(dict(fx["gs"])["G6"])
    top = g["G6"][0]
    assert top["keys"] == [5, 6] and top["batch_genome"] == 5 and top["genome_id"] == "G6"
    assert top["score"] == per[5]["score"] + per[6]["score"] and top["score2"] == sum(per[5]["longest"])
    assert sum(1 for r in g["G6"] if r["genome_id"] == "G6") == 1
    assert g["short"] == [] and all(r["score2"] < 0.8 * g["G1"][0]["score2"] for r in g["unrelated"])
    # G4: the missing-prefix rule in the query, the outlier lists in the index
    assert fx["gi"].info()["outlier_seeds"] > 0 and g["G4"][0]["hit_masks"] > 0.8 * fx["M"]


def test_details_off_and_the_cut(fx):
    qs, exp = fx["qs"], fx["exp"]
    plain = fx["gi"].screen(qs, details=False, top_n=0)
    assert [[(r["keys"], r["score"], r["batch_genome"]) for r in q] for q in plain] == \
           [[(r["keys"], r["score"], r["batch_genome"]) for r in q] for q in exp]
    assert all(r["score2"] == r["hit_masks"] == r["hit_kmers"] == 0 and r["prefixes"] == [] for q in plain for r in q)
    _same(plain, fx["model"].screen(qs, details=False, top_n=0))
    for n in (1, 3):
        _same(fx["gi"].screen(qs, details=True, top_n=n), [q[:n] for q in exp])
    # at the lowest min_prefix chance matches give every query more rows than the cut keeps
    info = fx["gi"].info()
    lo = info["mask_prefix"] + info["anchor_prefix"]
    exp_lo = fx["model"].screen(qs[:3], details=True, top_n=0, min_prefix=lo)
    assert min(len(q) for q in exp_lo) > 3
    for n in (1, 3):
        _same(fx["gi"].screen(qs[:3], details=True, top_n=n, min_prefix=lo), [q[:n] for q in exp_lo])
    _same(fx["gi"].screen(qs[:2], details=True), [q[:10] for q in exp[:2]])     # the default cut is 10


def test_three_windows(fx):
    qs = [fx["qs"][2], fx["qs"][0]]       # G2: regions, unshifted; G1
    exp = fx["model"].screen(qs, details=True, top_n=0, windows=3)
    _same(fx["gi"].screen(qs, details=True, top_n=0, windows=3), exp)
    assert _norm(exp) != _norm([fx["exp"][2], fx["exp"][0]])
    # more windows than the short query has k-mers for: windows shorter than k capture nothing
    q8 = [fx["qs"][6]]
    _same(fx["gi"].screen(q8, details=True, top_n=0, windows=9), fx["model"].screen(q8, details=True, top_n=0, windows=9))


def test_min_prefix_at_both_ends(fx):
    info = fx["gi"].info()
    lo = info["mask_prefix"] + info["anchor_prefix"]
    assert (lo, F.K) == fx["model"].min_prefix_range()
    qs = [fx["qs"][0], fx["qs"][4], fx["qs"][8]]
    for p in (lo, F.K):
        exp = fx["model"].screen(qs, details=True, top_n=0, min_prefix=p)
        _same(fx["gi"].screen(qs, details=True, top_n=0, min_prefix=p), exp)
    assert set(exp[0][0]["prefixes"]) == {F.K} and len(exp[2]) == 0
    assert len(fx["model"].screen(qs, details=True, top_n=0, min_prefix=lo)[2]) > 0


def tie_genomes():
    rng = random.Random(20261019)
    r = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))   # noqa: E731
    same = r(30_000)
    tandem = r(1000) + r(37) * 300 + r(1000)
    return [("TA", [("TA_c", same)]), ("TB", [("TB_c", same)]), ("TR", [("TR_c", tandem)])]


def test_ties_go_by_key_and_hits_saturate_at_255(fx):
    la = fx["la"]
    gs = tie_genomes()
    gi = la.Index.from_genomes(gs, la.BuildOpt.default(masks=1024))
    try:
        masks = gi.masks().tolist()
        d = str(fx["tmp"] / "ties.lmi")
        O.build_index(d, gs, O.default_build_opt(chunks=2, masks=1024), masks=masks)
        model = SM.Model(d, F.K, masks, [], {0: "TA", 1: "TB", 2: "TR"})
        try:
            per = model.per_record(gs[2][1])
            assert any(v > 255 and h == 255 for v, h in zip(per[2]["values"], per[2]["hits"]))   # the model saturates
            exp = model.screen(gs, details=True, top_n=0)
            assert [r["batch_genome"] for r in exp[0][:2]] == [0, 1] and exp[0][0]["score"] == exp[0][1]["score"]
            assert exp[2][0]["batch_genome"] == 2 and exp[2][0]["hit_kmers"] < sum(per[2]["values"])
            _same(gi.screen(gs, details=True, top_n=0), exp)
            _same(gi.screen(gs, details=False, top_n=1), model.screen(gs, details=False, top_n=1))
        finally:
            model.close()
    finally:
        gi.close()


def test_the_genome_whitelist_is_honoured(fx):
    gi, qs = fx["gi"], [fx["qs"][0], fx["qs"][5], fx["qs"][2]]
    keep = {7, 6}
    exp = fx["model"].screen(qs, details=True, top_n=0, keep=keep)
    gi.set_genome_filter(sorted(keep))
    try:
        got = gi.screen(qs, details=True, top_n=0)
    finally:
        gi.set_genome_filter([])
    _same(got, exp)
    assert [r["keys"] for r in exp[0]] == [[7]] and [r["keys"] for r in exp[1]][0] == [6]
    assert all(set(r["keys"]) <= keep for q in exp for r in q)
    _same(gi.screen(qs, details=True, top_n=0), [fx["exp"][0], fx["exp"][5], fx["exp"][2]])   # cleared


def test_small_pieces_change_nothing(fx):
    qs = [fx["qs"][0], fx["qs"][5]]
    _, whole = fx["gi"].screen(qs, details=True, top_n=0, want_stats=True)
    assert whole["pieces"] == 1 and whole["tuples"] > 40_000
    os.environ["LM_SCREEN_PIECE_TUPLES"] = "9000"
    try:
        got, st = fx["gi"].screen(qs, details=True, top_n=0, want_stats=True)
        plain = fx["gi"].screen(qs, details=False, top_n=0)
    finally:
        del os.environ["LM_SCREEN_PIECE_TUPLES"]
    assert st["pieces"] >= 4 and st["tuples"] == whole["tuples"]
    _same(got, [fx["exp"][0], fx["exp"][5]])
    assert [[(r["keys"], r["score"]) for r in q] for q in plain] == [[(r["keys"], r["score"]) for r in q] for q in got]


def test_other_ways_to_a_handle_give_the_same_rows(fx):
    la, qs = fx["la"], [fx["qs"][i] for i in (0, 5, 4, 6)]
    exp = [fx["exp"][i] for i in (0, 5, 4, 6)]
    oi = la.Index(fx["dir"])
    try:
        _same(oi.screen(qs, details=True, top_n=0), exp)
    finally:
        oi.close()
    saved = str(fx["tmp"] / "saved.lmi")
    fx["gi"].save(saved, chunks=3)
    si = la.Index(saved, residency=la.api.Residency(la.api.GENOMES_HOST))     # saved, opened, genomes in host memory
    try:
        assert si.residency()["genomes_host"] == 9
        _same(si.screen(qs, details=True, top_n=0), exp)
    finally:
        si.close()


def test_two_shards_together_give_the_unsharded_rows(fx):
    """The union of both ranks' rows at top_n = 0 equals the unsharded rows.  The reference's search starts from an anchor
    index in which a later run of k-mers with the same anchor bases hides an earlier one (screen_shadowed in lm_screen.hip),
    and such a run can belong to a record of the other shard - the k-mers tiny genomes (G4, G8) leave under masks whose
    prefix they lack.  So the ranks first exchange the structure of their lists (Index.screen_structure /
    add_screen_structure: occupied partitions and outlier k-mers, no values), once per index.  Without the exchange the
    union's sums are at least the unsharded ones and somewhere larger: asserted too, so that the exchange is what is tested.
    A refused blob leaves the handle as it was; None takes it back to its own lists."""
    la, qs = fx["la"], [fx["qs"][i] for i in (0, 5, 4, 6)]
    exp = _norm([fx["exp"][i] for i in (0, 5, 4, 6)])
    shards = [la.Index.from_genomes(fx["gs"], la.BuildOpt.default(max_genome=F.MAX_GENOME),
                                    options=la.api.default_options(shard_rank=r, shard_count=2)) for r in range(2)]

    def union():
        parts = [_norm(s.screen(qs, details=True, top_n=0)) for s in shards]
        assert all(sum(len(q) for q in p) > 0 for p in parts)
        return [sorted(parts[0][qi] + parts[1][qi], key=lambda r: (-r["score"], r["batch_genome"])) for qi in range(len(qs))]
    try:
        alone = union()
        assert [[r["keys"] for r in q] for q in alone] == [[r["keys"] for r in q] for q in exp]
        assert alone != exp and all(a["score"] >= e["score"] for qa, qe in zip(alone, exp) for a, e in zip(qa, qe))
        blobs = [s.screen_structure() for s in shards]
        shards[0].add_screen_structure(blobs[1])
        shards[1].add_screen_structure(blobs[0])
        both = union()
        for qi, (u, e) in enumerate(zip(both, exp)):
            assert u == e, (qi, [(r["batch_genome"], r["score"], r["hit_masks"]) for r in u], [(r["batch_genome"], r["score"], r["hit_masks"]) for r in e])
        # a structure of another index is refused, the handle keeps what it has; None takes it back to its own lists
        with pytest.raises(ValueError, match="structure"):
            shards[0].add_screen_structure(b"\0" * 64)
        with pytest.raises(ValueError, match="header"):
            shards[0].add_screen_structure(b"abc")
        # two k-mers of one outlier list swapped (the whole index's structure: most lists hold one of G4 and one of G8).
        # Blob: 40-byte header, bitmaps [2M][64] u64, offsets [2M + 1] i64, k-mers u64
        bad = bytearray(fx["gi"].screen_structure())
        nb, no = 2 * fx["M"] * 64 * 8, (2 * fx["M"] + 1) * 8
        offs = memoryview(bytes(bad[40 + nb:40 + nb + no])).cast("q")
        at = next(40 + nb + no + 8 * offs[i] for i in range(2 * fx["M"]) if offs[i + 1] - offs[i] >= 2 and
                  bad[40 + nb + no + 8 * offs[i]:][:8] != bad[40 + nb + no + 8 * offs[i] + 8:][:8])
        bad[at:at + 8], bad[at + 8:at + 16] = bad[at + 8:at + 16], bad[at:at + 8]
        with pytest.raises(ValueError, match="not ascending"):
            shards[0].add_screen_structure(bytes(bad))
        shards[0].add_screen_structure(blobs[1])                                   # adding one twice changes nothing
        assert union() == both
        for s in shards:
            s.add_screen_structure(None)
        assert union() == alone
        # the unsharded handle with its own structure added to itself: nothing changes
        fx["gi"].add_screen_structure(fx["gi"].screen_structure())
        try:
            _same(fx["gi"].screen(qs, details=True, top_n=0), exp)
        finally:
            fx["gi"].add_screen_structure(None)
    finally:
        for s in shards:
            s.close()


def test_k_21_with_three_masks_on_a_prefix(fx):
    la = fx["la"]
    k, ms = 21, MS.skewed(21, 24)
    assert max(MS.per_prefix(k, ms)) >= 3
    gi = la.Index.from_genomes(fx["gs"], la.BuildOpt.default(k=k, max_genome=F.MAX_GENOME), masks=ms)
    try:
        d = str(fx["tmp"] / "k21.lmi")
        O.build_index(d, fx["gs"], O.default_build_opt(k=k, chunks=2, max_genome=F.MAX_GENOME, masks=len(ms)), masks=list(ms))
        model = SM.Model(d, k, list(ms), SM.chunk_lists(fx["recs"]), fx["names"])
        try:
            qs = [fx["qs"][i] for i in (0, 2, 5, 6)]
            for p in (21, model.min_prefix_range()[0]):
                exp = model.screen(qs, details=True, top_n=0, min_prefix=p)
                _same(gi.screen(qs, details=True, top_n=0, min_prefix=p), exp)
            assert any(r["batch_genome"] == 0 for r in exp[0]) and any(r["keys"] == [5, 6] for r in exp[2])
        finally:
            model.close()
    finally:
        gi.close()


def test_refusals_leave_the_handle_usable(fx):
    la, gi = fx["la"], fx["gi"]
    L = la.lib()
    g1 = [fx["qs"][0]]
    info = gi.info()
    cases = [(dict(windows=0), "windows"), (dict(min_prefix=F.K + 1), "min_prefix"),
             (dict(min_prefix=info["mask_prefix"] + info["anchor_prefix"] - 1), "min_prefix")]
    for kw, word in cases:
        with pytest.raises(ValueError, match=word):
            gi.screen(g1, **kw)
    with pytest.raises(ValueError, match="no contigs"):
        gi.screen([("empty", [])])
    sc = C.c_void_p()
    opt = la.api.ScreenOpt(21, 0, 10, 0)
    q = (la.api.GenomeQuery * 1)()
    assert L.lm_index_screen_genomes(gi.h, q, 1, C.byref(opt), C.byref(sc)) == 7 and b"windows" in L.lm_last_error(gi.h)
    opt = la.api.ScreenOpt(F.K + 1, 1, 10, 0)
    assert L.lm_index_screen_genomes(gi.h, q, 1, C.byref(opt), C.byref(sc)) == 3 and b"min_prefix" in L.lm_last_error(gi.h)
    opt = la.api.ScreenOpt(21, 1, 10, 0)
    assert L.lm_index_screen_genomes(gi.h, None, 1, C.byref(opt), C.byref(sc)) == 7 and b"NULL" in L.lm_last_error(gi.h)
    assert L.lm_index_screen_genomes(gi.h, q, 1, C.byref(opt), C.byref(sc)) == 7 and b"no contigs" in L.lm_last_error(gi.h)
    # a query of 2^28 bases: lengths alone decide, before any byte is read
    big = b"A" * (1 << 27)
    cs = (la.api.Contig * 2)()
    for c in cs:
        c.id, c.seq, c.len = b"c", big, len(big)
    q[0].id, q[0].contigs, q[0].ncontigs = b"big", cs, 2
    assert L.lm_index_screen_genomes(gi.h, q, 1, C.byref(opt), C.byref(sc)) == 7 and b"2^28" in L.lm_last_error(gi.h)
    assert not sc.value
    assert L.lm_index_screen_genomes(gi.h, None, 0, None, C.byref(sc)) == 0 and L.lm_screen_rows(sc, None) == 0
    L.lm_screen_free(sc)
    # the handle screens and searches as before
    _same(gi.screen(g1, details=True, top_n=0), fx["exp"][:1])
    rows, _ = gi.search(F.queries(fx["gs"]))
    oi = O.Index(fx["dir"])
    try:
        exp = [(r["batch_genome"], r["qbegin"], r["qend"], r["tbegin"], r["tend"], r["bitscore"]) for q in F.queries(fx["gs"]) for r in oi.search(q)[0]]
    finally:
        oi.close()
    assert [(r["batch_genome"], r["qbegin"], r["qend"], r["tbegin"], r["tend"], r["bitscore"]) for r in rows] == exp and exp


def test_the_printer(fx):
    la = fx["la"]
    qs, ids = fx["qs"][:3] + fx["qs"][5:6], ["G1", "G7", "G2", "G6"]
    got = fx["gi"].screen(qs, details=True, top_n=3)
    exp = [q[:3] for q in fx["exp"][:3] + fx["exp"][5:6]]
    for extra in (False, True):
        lines = la.format_screen_rows(got, ids, 21, fx["M"], extra=extra, header=True)
        head = "query\tsubject\tminPrefix\tfracMasks\tnMasks\tsumPrefix\tavgPrefix" + ("\tprefixes" if extra else "")
        assert lines[0] == head
        assert lines[1:] == SM.format_rows(exp, ids, 21, fx["M"], extra=extra) and len(lines) > 6
    assert lines[1].split("\t")[:2] == ["G1", "G1"] and lines[1].split("\t")[6] == "31.00"
