"""Similar genome pairs on the GPU (lm_index_genome_pairs, Index.pairs) against the Python model over the oracle
(tests/pair_model.py): every comparison is exact, row for row and field for field, order included.  Indexes: the sets P and
C of tests/pair_fixture.py, built once per module by Index.from_genomes and by the oracle's writer with the same masks."""
import os

import pytest

import genome_build_fixture as F
import oracle as O
import pair_fixture as PF
import pair_model as PM

pytestmark = pytest.mark.gpu


def _rows(got):
    return [(r["key1"], r["key2"], r["n_masks"], r["sum_prefix"]) for r in got]


def _same(got, exp, names=None):
    g = _rows(got)
    assert len(g) == len(exp), (len(g), len(exp), g[:5], exp[:5])
    for i, (a, b) in enumerate(zip(g, exp)):
        assert a == b, (i, a, b)
    if names is not None:
        for r in got:
            assert (r["genome1"].decode(), r["genome2"].decode()) == (names[r["key1"]], names[r["key2"]])


def _oracle_model(tmp, name, gs, masks, **kw):
    d = str(tmp / name)
    O.build_index(d, gs, O.default_build_opt(chunks=3, masks=len(masks), **kw), masks=masks)
    return PM.Model(d, PF.K, masks)


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    import lexicmap_amd as la
    tmp = tmp_path_factory.mktemp("pairs")
    pg, pm, cg, cm = PF.p_genomes(), PF.p_masks(), PF.c_genomes(), PF.c_masks()
    bo_p = la.BuildOpt.default(max_genome=PF.P_MAX_GENOME)
    P = la.Index.from_genomes(pg, bo_p, masks=pm)
    Cx = la.Index.from_genomes(cg, la.BuildOpt.default(), masks=cm)
    out = dict(la=la, tmp=tmp, pg=pg, pm=pm, cg=cg, cm=cm, bo_p=bo_p, P=P, C=Cx,
               mP=_oracle_model(tmp, "P.lmi", pg, pm, max_genome=PF.P_MAX_GENOME), mC=_oracle_model(tmp, "C.lmi", cg, cm),
               p_names=dict(enumerate(PF.p_record_names())), c_names={i: g[0] for i, g in enumerate(cg)})
    yield out
    P.close()
    Cx.close()


# ---- 1. P against the model
def test_P_equals_the_model_over_prefixes_and_mask_counts(fx):
    P, m = fx["P"], fx["mP"]
    info = P.info()
    lo = info["mask_prefix"] + info["anchor_prefix"]
    assert (lo, PF.K) == m.min_prefix_range() and info["genomes"] == 11 and info["outlier_seeds"] > 0
    for p in (lo, 21, PF.K):
        for nm in (0, 64, 256, 1024):
            got, st = P.pairs(min_prefix=p, masks=nm, min_mask_fraction=0.0, want_stats=True)
            r = m.run(p, nm)
            _same(got, m.rows(p, nm, 0.0), fx["p_names"])
            assert st["total_masks"] == r["total"] and st["tuples"] == r["tuples"] and st["rows"] == len(got) == len(r["pairs"])
            assert st["required"] == 0 and st["pairs_seen"] == len(r["pairs"]) and st["pieces"] >= 1
    assert m.run(21, 1024)["total"] == 1024 < info["masks"] == 1500


def test_P_defaults_and_the_threshold_at_one_pairs_count(fx):
    P, m = fx["P"], fx["mP"]
    exp = m.rows()
    got, st = P.pairs(want_stats=True)
    _same(got, exp, fx["p_names"])
    assert st["total_masks"] == 1024 and st["required"] == 256 and 0 < len(exp) < len(m.rows(21, 1024, 0.0))
    assert _rows(got)[0][:3] == (0, 4, 1024) and _rows(got)[0][3] == 31 * 1024
    # the tie only the key order breaks: (A, A2) before (A2, Acopy)
    g = _rows(got)
    i = g.index((0, 1) + tuple(m.run(21, 1024)["pairs"][(0, 1)]))
    assert g[i + 1][:2] == (1, 4) and g[i + 1][2:] == g[i][2:]
    # required == one pair's n_masks keeps it, that value plus one drops it
    total = 1024
    n = m.run(21, 1024)["pairs"][(0, 9)][0]
    for want, kept in ((n, True), (n + 1, False)):
        f = next(x / 100000.0 for x in range(100001) if PM.required(x / 100000.0, total) == want)
        got = P.pairs(min_mask_fraction=f)
        _same(got, m.rows(21, 1024, f))
        assert ((0, 9) in [r[:2] for r in _rows(got)]) == kept


# ---- 2. C against the model: groups wider than two wavefronts, same-record seed pairs, pieces
def test_C_equals_the_model_in_one_piece_and_in_many(fx):
    Cx, m, la = fx["C"], fx["mC"], fx["la"]
    assert "LM_PAIR_PIECE_TUPLES" not in os.environ
    for nm in (64, 0):
        r = m.run(21, nm)
        assert r["largest_group"] > 128 and r["same_record"] >= 1
        base = {}
        for f in (0.0, 0.25):
            got, st = Cx.pairs(masks=nm, min_mask_fraction=f, want_stats=True)
            _same(got, m.rows(21, nm, f), fx["c_names"] if f else None)
            assert st["tuples"] == r["tuples"] and st["total_masks"] == r["total"]
            base[f] = _rows(got)
        try:
            for piece, least in ((r["tuples"] // 10, 8), (1, r["total"] // 2)):     # about ten pieces; one-mask pieces only
                os.environ["LM_PAIR_PIECE_TUPLES"] = str(piece)
                for f in (0.0, 0.25):
                    got, st = Cx.pairs(masks=nm, min_mask_fraction=f, want_stats=True)
                    assert _rows(got) == base[f]
                    assert st["pieces"] > 1 and st["pieces"] >= least and st["tuples"] == r["tuples"]
        finally:
            del os.environ["LM_PAIR_PIECE_TUPLES"]


# ---- 3. keys
def test_a_selection_of_records(fx):
    P, m = fx["P"], fx["mP"]
    sel = [9, 0, 4, 5, 10, 7, 1]
    got, st = P.pairs(keys=sel, min_mask_fraction=0.0, want_stats=True)
    _same(got, m.rows(21, 1024, 0.0, keys=sel), fx["p_names"])
    assert st["tuples"] == m.run(21, 1024, sel)["tuples"] and len(got) > 3
    _same(P.pairs(keys=sel, masks=0), m.rows(21, 0, 0.25, keys=sel))
    assert P.pairs(keys=[]) == [] and P.pairs(keys=[3]) == []
    for bad in ([0, 99], [1 << 20], [0, 4, 0]):
        with pytest.raises(ValueError):
            P.pairs(keys=bad)
    _same(P.pairs(), m.rows())


# ---- 4. handles
def test_saved_joined_subset_and_host_resident_handles(fx):
    la, P, m, tmp, pg, pm, bo = fx["la"], fx["P"], fx["mP"], fx["tmp"], fx["pg"], fx["pm"], fx["bo_p"]
    exp0 = m.rows(21, 0, 0.0)
    opened = []
    try:
        path = str(tmp / "P_saved.lmi")
        P.save(path, chunks=3)
        o = la.Index(path)
        opened.append(o)
        _same(o.pairs(masks=0, min_mask_fraction=0.0), exp0, fx["p_names"])
        _same(o.pairs(), m.rows())
        a, b = la.Index.from_genomes(pg[:5], bo, masks=pm), la.Index.from_genomes(pg[5:], bo, masks=pm)
        opened += [a, b]
        j = a.join(b)
        opened.append(j)
        _same(j.pairs(masks=0, min_mask_fraction=0.0), exp0, fx["p_names"])
        _same(j.pairs(min_prefix=m.min_prefix_range()[0], min_mask_fraction=0.0), m.rows(m.min_prefix_range()[0], 1024, 0.0))
        keep = [0, 1, 4, 5, 9]                                  # A, A2, Acopy, tiny, half: renumbered 0 .. 4
        sub = P.subset(keep)
        opened.append(sub)
        names = PF.p_record_names()
        d = dict(pg)
        ms = _oracle_model(tmp, "P_sub.lmi", [(names[k], d[names[k]]) for k in keep], pm, max_genome=PF.P_MAX_GENOME)
        _same(sub.pairs(masks=0, min_mask_fraction=0.0), ms.rows(21, 0, 0.0), {i: names[k] for i, k in enumerate(keep)})
        _same(sub.pairs(), ms.rows())
        assert len(ms.rows(21, 0, 0.0)) >= 6
        h = la.Index.from_genomes(pg, bo, residency=la.api.Residency(la.api.GENOMES_HOST), masks=pm)
        opened.append(h)
        assert h.residency()["genomes_device"] == 0
        _same(h.pairs(masks=0, min_mask_fraction=0.0), exp0, fx["p_names"])
    finally:
        for ix in opened:
            ix.close()


# ---- 5. the builder tests' genome set with its generated 20 000 masks
def test_the_builder_fixture_with_generated_masks(fx):
    la, tmp = fx["la"], fx["tmp"]
    gs = F.genomes()
    gi = la.Index.from_genomes(gs, la.BuildOpt.default(max_genome=F.MAX_GENOME))
    try:
        masks = gi.masks().tolist()
        d = str(tmp / "builder.lmi")
        O.build_index(d, gs, O.default_build_opt(chunks=4, max_genome=F.MAX_GENOME), masks=masks)
        m = PM.Model(d, F.K, masks)
        names = {i: r[0] for i, r in enumerate(F.records(gs))}
        _same(gi.pairs(), m.rows(), names)
        _same(gi.pairs(min_mask_fraction=0.0), m.rows(21, 1024, 0.0), names)
        assert len(m.rows(21, 1024, 0.0)) >= 1
    finally:
        gi.close()


# ---- 6. refusals leave the handle usable
def test_refusals_leave_the_handle_answering(fx):
    la, P, m = fx["la"], fx["P"], fx["mP"]
    lo = m.min_prefix_range()[0]
    exp = m.rows()
    L = la.lib()
    for kw, word in ((dict(min_prefix=lo - 1), "min_prefix"), (dict(min_prefix=PF.K + 1), "min_prefix"), (dict(masks=100), "masks"),
                     (dict(masks=16), "masks"), (dict(masks=-64), "masks"), (dict(masks=4096), "masks"),
                     (dict(min_mask_fraction=-0.1), "min_mask_fraction"), (dict(min_mask_fraction=float("nan")), "min_mask_fraction"),
                     (dict(keys=[0, 77]), "no record"), (dict(keys=[2, 2]), "twice")):
        with pytest.raises(ValueError) as e:
            P.pairs(**kw)
        assert word in str(e.value), (kw, str(e.value))
        _same(P.pairs(), exp)
    # the statuses behind the ValueErrors: 3 for options, 7 for arguments
    import ctypes as C
    pr = C.c_void_p()
    assert L.lm_index_genome_pairs(P.h, None, 0, C.byref(la.PairOpt(5, 1024, 0.25)), C.byref(pr)) == 3 and not pr.value
    one = (C.c_uint64 * 1)(500)
    assert L.lm_index_genome_pairs(P.h, one, 1, None, C.byref(pr)) == 7 and not pr.value
    assert L.lm_index_genome_pairs(P.h, None, 3, None, C.byref(pr)) == 7 and not pr.value
    # a shard cannot see the pairs across shards
    sh = la.Index.from_genomes(fx["pg"], fx["bo_p"], options=la.api.default_options(shard_rank=0, shard_count=2), masks=fx["pm"])
    try:
        with pytest.raises(ValueError) as e:
            sh.pairs()
        assert "shard" in str(e.value)
        assert len(sh.seed_positions()) == sh.info()["genomes"]      # the shard still answers
    finally:
        sh.close()
    _same(P.pairs(), exp)


# ---- 7. formatter
def test_formatted_lines_equal_pythons(fx):
    la, P, m = fx["la"], fx["P"], fx["mP"]
    for p, nm, f in ((21, 1024, 0.25), (m.min_prefix_range()[0], 0, 0.0)):
        got, st = P.pairs(min_prefix=p, masks=nm, min_mask_fraction=f, want_stats=True)
        lines = la.format_pair_rows(got, p, st["total_masks"], header=True)
        assert lines == [PM.HEADER] + PM.format_rows(m.rows(p, nm, f), fx["p_names"], p, m.run(p, nm)["total"])
    assert any("\t1.0000\t" in l for l in lines)                    # A and Acopy: n_masks == total
    arr = P.pairs(arrays=True)
    assert [tuple(int(x) for x in r) for r in arr] == m.rows() and arr.dtype.names == ("key1", "key2", "n_masks", "sum_prefix")
