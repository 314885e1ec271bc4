"""Similar genome pairs across the shards of a sharded index (lm_index_pair_seeds, lm_index_genome_pairs_across,
lm_pairs_merge; Index.pair_seeds, Index.pairs_across, merge_pair_rows): rank r pairs its own records among themselves and with
the records of the ranks s < r, whose seed blobs it is given; the merge of all ranks' rows must be the unsharded index's
Index.pairs row for row and field for field, names included, and equal the Python model over the oracle (tests/pair_model.py).
Indexes: the sets P and C of tests/pair_fixture.py, unsharded and as shards, built once per module."""
import os
import struct

import pytest

import mask_sets as MS
import oracle as O
import pair_fixture as PF
import pair_model as PM

pytestmark = pytest.mark.gpu


def _rows(got):
    return [(r["key1"], r["key2"], r["n_masks"], r["sum_prefix"]) for r in got]


def _keys(ix):
    return [int(k) for k in ix.seed_distances()["records"]["key"]]


def _shard_opt(la, r, n):
    return la.api.default_options(shard_rank=r, shard_count=n)


def _union(la, shards, want_stats=False, blobs=None, **kw):
    """every rank exports once (per mask selection), rank r takes the blobs of the ranks s < r, rank 0 merges"""
    blobs = blobs or [s.pair_seeds(masks=kw.get("masks", 1024)) for s in shards]
    parts = [s.pairs_across(blobs[:r], want_stats=True, **kw) for r, s in enumerate(shards)]
    merged = la.merge_pair_rows([p[0] for p in parts])
    return (merged, [p[1] for p in parts]) if want_stats else merged


def _own_rows(rows, own):
    own = set(own)
    return [r for r in rows if r["key1"] in own or r["key2"] in own]


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    import lexicmap_amd as la
    tmp = tmp_path_factory.mktemp("pairs_shards")
    pg, pm, cg, cm = PF.p_genomes(), PF.p_masks(), PF.c_genomes(), PF.c_masks()
    bo_p = la.BuildOpt.default(max_genome=PF.P_MAX_GENOME)
    out = dict(la=la, tmp=tmp, pg=pg, pm=pm, cg=cg, cm=cm, bo_p=bo_p)
    out["P"] = la.Index.from_genomes(pg, bo_p, masks=pm)
    out["C"] = la.Index.from_genomes(cg, la.BuildOpt.default(), masks=cm)
    out["Ps"] = {n: [la.Index.from_genomes(pg, bo_p, options=_shard_opt(la, r, n), masks=pm) for r in range(n)] for n in (2, 3)}
    out["Cs"] = [la.Index.from_genomes(cg, la.BuildOpt.default(), options=_shard_opt(la, r, 2), masks=cm) for r in range(2)]
    d = str(tmp / "P.lmi")
    O.build_index(d, pg, O.default_build_opt(chunks=3, masks=len(pm), max_genome=PF.P_MAX_GENOME), masks=pm)
    out["mP"] = PM.Model(d, PF.K, pm)
    yield out
    for ix in [out["P"], out["C"]] + out["Cs"] + [s for ss in out["Ps"].values() for s in ss]:
        ix.close()


# ---- 1. the union of the ranks' rows is the unsharded result
def test_union_equals_unsharded_and_the_model_on_P(fx):
    la, P, m = fx["la"], fx["P"], fx["mP"]
    info = P.info()
    lo = info["mask_prefix"] + info["anchor_prefix"]
    assert info["genomes"] == 11 and lo < 21
    for n, shards in fx["Ps"].items():
        held = [_keys(s) for s in shards]
        assert sorted(k for h in held for k in h) == list(range(11)) and all(held)
        assert sum(1 for h in held if 6 in h and 7 in h) == 1                   # the split genome S: whole on one shard
    shard_of = {n: {k: r for r, s in enumerate(shards) for k in _keys(s)} for n, shards in fx["Ps"].items()}
    seen_rows = seen_cross = 0
    for nm in (0, 64, 256):
        blobs = {n: [s.pair_seeds(masks=nm) for s in shards] for n, shards in fx["Ps"].items()}   # (no other option is in a blob)
        for p in (lo, 21, PF.K):
            for f in (0.0, 0.25, 0.9):
                exp = P.pairs(min_prefix=p, masks=nm, min_mask_fraction=f)
                assert _rows(exp) == m.rows(p, nm, f)
                for n, shards in fx["Ps"].items():
                    got = _union(la, shards, blobs=blobs[n], min_prefix=p, masks=nm, min_mask_fraction=f)
                    assert got == exp, (n, p, nm, f, _rows(got)[:4], _rows(exp)[:4])
                    seen_cross += sum(1 for r in got if shard_of[n][r["key1"]] != shard_of[n][r["key2"]])
                seen_rows += len(exp)
    assert seen_rows > 100 and seen_cross > 100
    names = dict(enumerate(PF.p_record_names()))
    for r in _union(la, fx["Ps"][3]):
        assert (r["genome1"].decode(), r["genome2"].decode()) == (names[r["key1"]], names[r["key2"]])


# ---- 2. C: one group of 130 identical records split 65 / 65, two seeds of one record in a group; pieces
def test_C_in_one_piece_and_in_many(fx):
    la, Cx, shards = fx["la"], fx["C"], fx["Cs"]
    held = [set(_keys(s)) for s in shards]
    assert [len(h & set(range(130))) for h in held] == [65, 65]
    assert (136 in held[0]) != (137 in held[0])                                  # rep and rep2 on different shards
    assert "LM_PAIR_PIECE_TUPLES" not in os.environ
    for nm in (64, 0):
        base, tuples = {}, None
        for f in (0.0, 0.25):
            exp, st = Cx.pairs(masks=nm, min_mask_fraction=f, want_stats=True)
            got, sts = _union(la, shards, want_stats=True, masks=nm, min_mask_fraction=f)
            assert got == exp and len(exp) >= 130 * 129 // 2
            # every unordered pair of entries of a group is emitted on exactly one rank
            assert sum(s["tuples"] for s in sts) == st["tuples"] > 0
            assert sum(s["entries"] for s in sts) == st["entries"] + sts[0]["entries"]   # rank 1 counts rank 0's again
            base[f], tuples = exp, st["tuples"]
        try:
            for piece, least in ((tuples // 20, 4), (1, (nm or len(fx["cm"])) // 2)):      # a few pieces; one-mask pieces only
                os.environ["LM_PAIR_PIECE_TUPLES"] = str(piece)
                for f in (0.0, 0.25):
                    got, sts = _union(la, shards, want_stats=True, masks=nm, min_mask_fraction=f)
                    assert got == base[f]
                    assert all(s["pieces"] >= least for s in sts) and sum(s["tuples"] for s in sts) == tuples
        finally:
            del os.environ["LM_PAIR_PIECE_TUPLES"]


# ---- 3. lopsided groups through keys, on the unsharded handle
def test_lopsided_groups_through_keys(fx):
    la, Cx = fx["la"], fx["C"]
    clones = list(range(130))
    kw = dict(masks=64, min_mask_fraction=0.0)
    for own, other in (([7], clones[:7] + clones[8:]), (clones[:64] + clones[65:], [64]), ([136, 137], clones[:6]), ([3, 9, 131], [])):
        blob = Cx.pair_seeds(keys=other, masks=64)
        got = Cx.pairs_across([blob], keys=own, **kw)
        exp = _own_rows(Cx.pairs(keys=own + other, **kw), own)
        assert got == exp, (own[:3], other[:3], len(got), len(exp))
        if len(own) == 1:
            assert len(got) == 129
        if len(other) == 1:
            assert len(got) == 129 * 128 // 2 + 129
    # rep and rep2 share no group with the clones: no cross rows, the pair of the two stays
    got = Cx.pairs_across([Cx.pair_seeds(keys=clones[:6], masks=64)], keys=[136, 137], **kw)
    assert [r[:2] for r in _rows(got)] == [(136, 137)]
    # an empty blob (a shard or a selection without records), no blobs at all, an empty own selection
    empty = Cx.pair_seeds(keys=[], masks=64)
    assert len(empty) == 56 + 65 * 8 and struct.unpack_from("<qq", empty, 32) == (0, 0)
    exp = Cx.pairs(keys=[3, 9, 131], **kw)
    assert Cx.pairs_across([empty], keys=[3, 9, 131], **kw) == exp == Cx.pairs_across([], keys=[3, 9, 131], **kw) and len(exp) == 3
    assert Cx.pairs_across([Cx.pair_seeds(keys=clones, masks=64)], keys=[], **kw) == []
    assert Cx.pairs_across([], **kw) == Cx.pairs(**kw)


# ---- 4. other kinds of handle
def test_loader_shards_host_resident_and_extended_shards(fx):
    la, P, pg, pm, bo, tmp = fx["la"], fx["P"], fx["pg"], fx["pm"], fx["bo_p"], fx["tmp"]
    opened = []
    try:
        exp0, exp = P.pairs(masks=0, min_mask_fraction=0.0), P.pairs()
        path = str(tmp / "P_saved.lmi")
        P.save(path, chunks=3)
        loaded = [la.Index(path, options=_shard_opt(la, r, 2)) for r in range(2)]
        opened += loaded
        assert sorted(_keys(loaded[0]) + _keys(loaded[1])) == list(range(11))
        assert _union(la, loaded, masks=0, min_mask_fraction=0.0) == exp0 and _union(la, loaded) == exp
        host = la.Index.from_genomes(pg, bo, options=_shard_opt(la, 0, 2), residency=la.api.Residency(la.api.GENOMES_HOST), masks=pm)
        opened.append(host)
        assert host.residency()["genomes_device"] == 0
        base = la.Index.from_genomes(pg[:5], bo, options=_shard_opt(la, 1, 2), masks=pm)
        opened.append(base)
        ext = base.extend(pg[5:], la.BuildOpt.default(max_genome=PF.P_MAX_GENOME, masks=len(pm)))   # (S is split as in P)
        opened.append(ext)
        assert _keys(ext) == _keys(fx["Ps"][2][1])
        assert _union(la, [host, ext], masks=0, min_mask_fraction=0.0) == exp0
        assert _union(la, [ext, host]) == exp                                    # which shard is "rank 0" does not matter
        assert _union(la, [loaded[0], ext]) == exp
    finally:
        for ix in opened:
            ix.close()


# ---- 5. refusals leave the handle answering
def test_refusals_leave_the_handle_answering(fx):
    la, P, pg, pm, bo = fx["la"], fx["P"], fx["pg"], fx["pm"], fx["bo_p"]
    s0, s1 = fx["Ps"][2]
    own = _keys(s1)
    within = [r for r in P.pairs(min_mask_fraction=0.0) if r["key1"] in own and r["key2"] in own]
    assert len(within) >= 2
    b0, b0_64 = s0.pair_seeds(masks=256), s0.pair_seeds(masks=64)
    other = la.Index.from_genomes(pg[:2], bo, masks=MS.skewed(PF.K, 1500, seed=2))
    try:
        foreign = other.pair_seeds(masks=256)
    finally:
        other.close()
    ns = 256
    off = 56 + len(_keys(s0)) * 10 + sum(len(PF.p_record_names()[k]) for k in _keys(s0))
    a, b = struct.unpack_from("<qq", b0, off + 8 * 100)
    assert a < b
    swapped = b0[:off + 800] + struct.pack("<qq", b, a) + b0[off + 816:]
    assert struct.unpack_from("<q", b0, off + 8 * ns)[0] == struct.unpack_from("<q", b0, 40)[0] > 0    # (the offsets are where the layout says)
    for blobs, kw, words in (([foreign], dict(masks=256), ("blob 0", "mask")),
                             ([b0_64], dict(masks=256), ("blob 0", "masks = 64")),
                             ([b0[:-5]], dict(masks=256), ("blob 0", "length")),
                             ([b0[:40]], dict(masks=256), ("blob 0", "shorter")),
                             ([swapped], dict(masks=256), ("blob 0", "monotone")),
                             ([s1.pair_seeds(masks=256)], dict(masks=256), ("own record",)),
                             ([b0, b0], dict(masks=256), ("blob 0", "blob 1")),
                             ([b0], dict(masks=256, min_prefix=5), ("min_prefix",)),
                             ([b0], dict(masks=100), ("masks",))):
        with pytest.raises(ValueError) as e:
            s1.pairs_across(blobs, **kw)
        assert all(w in str(e.value) for w in words), (words, str(e.value))
        assert s1.pairs_across([], min_mask_fraction=0.0) == within                                     # the within-shard rows, which pairs() refuses
    assert s1.pairs_across([b0], masks=256) == _own_rows(P.pairs(masks=256), own)
    for sh in (s0, s1):
        with pytest.raises(ValueError) as e:
            sh.pairs()
        assert "shard" in str(e.value)
    with pytest.raises(ValueError) as e:
        s1.pair_seeds(keys=[_keys(s0)[0]])
    assert "another shard" in str(e.value)
    # the statuses behind the ValueErrors: 7 for arguments, also for blobs == NULL with nblobs > 0
    import ctypes as C
    pr = C.c_void_p()
    assert la.lib().lm_index_genome_pairs_across(s1.h, None, 0, None, None, 2, None, C.byref(pr)) == 7 and not pr.value
    assert "NULL" in la.lib().lm_last_error(s1.h).decode()
    assert s1.pairs_across([], min_mask_fraction=0.0) == within


# ---- 6. merge
def test_merge_in_any_order_and_the_formatted_lines(fx):
    la, P = fx["la"], fx["P"]
    shards = fx["Ps"][3]
    exp, st = P.pairs(min_mask_fraction=0.0, want_stats=True)
    blobs = [s.pair_seeds() for s in shards]
    parts = [s.pairs_across(blobs[:r], min_mask_fraction=0.0) for r, s in enumerate(shards)]
    assert sum(1 for p in parts if p) >= 2
    for order in ((0, 1, 2), (2, 1, 0), (1, 2, 0)):
        assert la.merge_pair_rows([parts[i] for i in order]) == exp
    assert la.merge_pair_rows(parts + [[]]) == exp
    lines = la.format_pair_rows(la.merge_pair_rows(parts), 21, st["total_masks"], header=True)
    assert lines == la.format_pair_rows(exp, 21, st["total_masks"], header=True) and len(lines) == len(exp) + 1
    # a rank that also took the blob of a HIGHER rank computed pairs that belong to that rank: refused by the merge
    wrong = shards[0].pairs_across([blobs[1]], min_mask_fraction=0.0)
    assert len(wrong) > len(parts[0])
    with pytest.raises(ValueError) as e:
        la.merge_pair_rows([wrong, parts[1], parts[2]])
    assert "twice" in str(e.value)
