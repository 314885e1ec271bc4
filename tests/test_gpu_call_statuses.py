"""The statuses of the eleven resident-index entry points that share one call guard (lm::guarded, lexicmap_amd/csrc/lm_internal.h;
the table in INTEGRATION.md), on an index of four genomes of a few kb.  For every entry point: a valid call, then calls the
library refuses on the host before any kernel runs - the numeric status (7 = LM_ERR_ARG, 3 = LM_ERR_OPTION where the call
checks an option) and a distinctive part of the text - then the valid call again, which must return what it returned before:
the handle's lock was given back and the handle is as usable as it was.  The one exception is lm_index_screen_structure: no
argument of a caller reaches a check inside it, so its only refusal is the NULL place for the answer, which is decided
before the lock and carries no text.  No call here exhausts, faults or waits for anything;
the LM_ERR_NOMEM answers are checked on the host (test_call_guard_cpu.py)."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG, OPTION = 7, 3
NO_KEY = 5 << 17   # batch 5 of an index that has one batch


def genomes():
    rng = random.Random(20261101)
    r = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))   # noqa: E731
    a = r(5000)
    near = bytearray(a)
    for i in range(0, len(near), 50):
        near[i] = ord("A") if near[i] != ord("A") else ord("C")
    return [("SA", [("SA_c", a)]), ("SB", [("SB_1", r(3000)), ("SB_2", r(2500))]), ("SN", [("SN_c", bytes(near))]), ("SC", [("SC_c", r(4000))])]


@pytest.fixture(scope="module")
def fx():
    import lexicmap_amd as la
    gs = genomes()
    gi = la.Index.from_genomes(gs, la.BuildOpt.default(masks=1024))
    yield dict(la=la, L=la.api.lib(), gs=gs, gi=gi)
    gi.close()


def refused(call, status, *words):
    """the binding raises ValueError for a refusal, with the library's text and the status"""
    with pytest.raises(ValueError) as e:
        call()
    assert e.value.status == status, (e.value.status, str(e.value))
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def raw_refused(fx, st, status, *words):
    """a call made past the binding (a NULL array with a count): the status and the text on the handle"""
    assert st == status
    text = fx["L"].lm_last_error(fx["gi"].h).decode()
    for w in words:
        assert w in text, (w, text)


def test_screen_genomes(fx):
    gi, qs = fx["gi"], fx["gs"][:2]
    before = gi.screen(qs, details=True, top_n=0)
    assert b"SA" in {r["genome_id"] for r in before[0]} and b"SB" in {r["genome_id"] for r in before[1]}
    refused(lambda: gi.screen(qs, windows=0), ARG, "lm_index_screen_genomes: windows = 0, needs to be > 0")
    refused(lambda: gi.screen(qs, top_n=-1), ARG, "top_n = -1 is negative")
    refused(lambda: gi.screen(qs, min_prefix=99), OPTION, "min_prefix (99) should be in the range of [")
    refused(lambda: gi.screen([("empty", [])]), ARG, "query 0 (empty) has no contigs")
    sc = C.c_void_p(1)
    raw_refused(fx, fx["L"].lm_index_screen_genomes(gi.h, None, 2, None, C.byref(sc)), ARG, "queries is NULL but nq is not 0")
    assert sc.value is None   # cleared before the work, set on LM_OK only
    assert gi.screen(qs, details=True, top_n=0) == before


def test_screen_structure_and_add_structure(fx):
    gi, L, qs = fx["gi"], fx["L"], fx["gs"][:2]
    blob = gi.screen_structure()
    rows = gi.screen(qs, top_n=0)
    assert len(blob) > 56 and gi.add_screen_structure(None) is None
    # lm_index_screen_structure refuses nothing but a NULL place for its answer, before it takes the lock and without a text
    n = C.c_size_t(7)
    assert L.lm_index_screen_structure(gi.h, None, C.byref(n)) == ARG
    refused(lambda: gi.add_screen_structure(blob[:20]), ARG, "lm_index_screen_add_structure: the blob is shorter than its header")
    refused(lambda: gi.add_screen_structure(b"\x01" + blob[1:]), ARG, "not a structure of lm_index_screen_structure")
    refused(lambda: gi.add_screen_structure(blob[:-8]), ARG, "the blob's length does not fit its header")
    assert gi.screen_structure() == blob
    assert gi.add_screen_structure(None) is None
    assert gi.screen(qs, top_n=0) == rows     # a refused blob left the handle with its own lists


def test_genome_pairs(fx):
    gi = fx["gi"]
    before = gi.pairs(min_mask_fraction=0.0)
    assert any({r["genome1"], r["genome2"]} == {b"SA", b"SN"} for r in before)
    refused(lambda: gi.pairs(keys=[0, NO_KEY]), ARG, "lm_index_genome_pairs: key %d (batch 5, index 0) is no record of this index" % NO_KEY)
    refused(lambda: gi.pairs(keys=[1, 1]), ARG, "is given twice")
    refused(lambda: gi.pairs(min_prefix=99), OPTION, "lm_index_genome_pairs: min_prefix (99) should be in the range of [")
    refused(lambda: gi.pairs(masks=100), OPTION, "lm_index_genome_pairs: ")
    refused(lambda: gi.pairs(min_mask_fraction=-0.5), OPTION, "should be >= 0")
    pr = C.c_void_p(1)
    raw_refused(fx, fx["L"].lm_index_genome_pairs(gi.h, None, 3, None, C.byref(pr)), ARG, "lm_index_genome_pairs: keys is NULL but nkeys is not 0")
    assert pr.value is None
    assert gi.pairs(min_mask_fraction=0.0) == before


def test_pair_seeds_and_genome_pairs_across(fx):
    gi = fx["gi"]
    blob = gi.pair_seeds(keys=[2, 3], masks=256)
    kw = dict(keys=[0, 1], masks=256, min_mask_fraction=0.0)
    before = gi.pairs_across([blob], **kw)
    assert any({r["genome1"], r["genome2"]} == {b"SA", b"SN"} for r in before)
    # lm_index_pair_seeds
    refused(lambda: gi.pair_seeds(keys=[NO_KEY], masks=256), ARG, "lm_index_pair_seeds: key %d" % NO_KEY, "is no record of this index")
    refused(lambda: gi.pair_seeds(masks=100), OPTION, "lm_index_pair_seeds: ")
    refused(lambda: gi.pair_seeds(masks=-4), OPTION, "masks (-4) should be 0 (all masks) or a power of 4 that is >= 64")
    assert gi.pair_seeds(keys=[2, 3], masks=256) == blob
    # lm_index_genome_pairs_across: a blob refused while it is parsed, and refusals of the call proper
    refused(lambda: gi.pairs_across([blob[:40]], **kw), ARG, "lm_index_genome_pairs_across: blob 0: its 40 bytes are shorter than the header")
    refused(lambda: gi.pairs_across([blob[:-5]], **kw), ARG, "blob 0: ", "length")
    refused(lambda: gi.pairs_across([blob], keys=[0, NO_KEY], masks=256), ARG, "lm_index_genome_pairs_across: key %d" % NO_KEY)
    refused(lambda: gi.pairs_across([blob], keys=[2], masks=256), ARG, "lm_index_genome_pairs_across: ")   # record 2 is the blob's too
    refused(lambda: gi.pairs_across([blob], keys=[0, 1], masks=256, min_prefix=5), OPTION, "min_prefix (5) should be in the range of [")
    assert gi.pairs_across([blob], **kw) == before


def test_seed_positions_and_distances(fx):
    gi, L = fx["gi"], fx["L"]
    pos = gi.seed_positions([1, 0])
    dist = gi.seed_distances([1, 0], min_dist=100, bins=8, bin_width=50)
    assert len(pos) == 2 and len(pos[0]) > 0 and len(dist["records"]) == 2
    sp = C.c_void_p(1)
    raw_refused(fx, L.lm_index_seed_positions(gi.h, None, 3, C.byref(sp)), ARG, "lm_index_seed_positions: keys is NULL but nkeys is not 0")
    assert sp.value is None
    refused(lambda: gi.seed_positions([0, NO_KEY]), ARG, "lm_index_seed_positions: key %d (batch 5, index 0) is no record of this index" % NO_KEY)
    refused(lambda: gi.seed_positions([3, 3]), ARG, "is given twice")
    refused(lambda: gi.seed_distances([0], bins=5, bin_width=0), ARG, "lm_index_seed_distances: hist_bins = 5 with hist_width < 1")
    refused(lambda: gi.seed_distances([0], bins=5000, bin_width=1), ARG, "hist_bins = 5000 (at most 4096 counters)")
    refused(lambda: gi.seed_distances([NO_KEY]), ARG, "lm_index_seed_distances: key %d" % NO_KEY)
    again = gi.seed_positions([1, 0])
    assert len(again) == 2 and all(np.array_equal(a, b) for a, b in zip(again, pos))
    d2 = gi.seed_distances([1, 0], min_dist=100, bins=8, bin_width=50)
    assert all(np.array_equal(d2[k], dist[k]) for k in ("records", "hist", "rows"))


def test_subseqs_subseq_rows_and_genome_seqs(fx):
    la, gi, L, gs = fx["la"], fx["gi"], fx["L"], fx["gs"]
    from lexicmap_amd.merge import ROW_DTYPE
    regions = [dict(key=0, seq_idx=0, begin=11, end=75), dict(genome_id="SB", seq_id="SB_2", begin=1, end=40, rc=1)]
    rows = np.zeros(2, dtype=ROW_DTYPE)
    rows["batch_genome"], rows["seq_idx"], rows["tbegin"], rows["tend"] = [0, 1], [0, 1], [10, 0], [74, 39]
    sub, by_rows, whole = gi.subseq(regions, 3, 3), gi.subseq_rows(rows), gi.genome_seqs("SB")
    assert sub.seqs[0] == gs[0][1][0][1][7:78] and by_rows.seqs == [gs[0][1][0][1][10:75], gs[1][1][1][1][:40]]
    assert whole.seqs == [gs[1][1][0][1], gs[1][1][1][1]]
    opt, sp = la.api.SubseqOpt(0, 0, 0, 0), C.c_void_p(1)
    # lm_index_subseqs
    raw_refused(fx, L.lm_index_subseqs(gi.h, None, 2, C.byref(opt), C.byref(sp)), ARG, "lm_index_subseqs: regions is NULL but n is not 0")
    assert sp.value is None
    refused(lambda: gi.subseq([dict(key=0, seq_idx=0, begin=5, end=4)]), ARG, "lm_index_subseqs: region 0: begin position")
    refused(lambda: gi.subseq([regions[0], dict(key=NO_KEY, seq_idx=0, begin=1, end=5)]), ARG, "lm_index_subseqs: region 1", "the genome is not in this index")
    refused(lambda: gi.subseq(regions, -1, 0), ARG, "upstream and downstream")
    # lm_index_subseq_rows
    sp = C.c_void_p(1)
    raw_refused(fx, L.lm_index_subseq_rows(gi.h, None, 2, C.byref(opt), C.byref(sp)), ARG, "lm_index_subseq_rows: rows is NULL but n is not 0")
    assert sp.value is None
    bad = rows.copy()
    bad["batch_genome"][1] = NO_KEY
    refused(lambda: gi.subseq_rows(bad), ARG, "lm_index_subseq_rows: region 1", "the genome is not in this index")
    # lm_index_genome_seqs
    refused(lambda: gi.genome_seqs("S9"), ARG, "lm_index_genome_seqs: reference name not found: S9")
    sp = C.c_void_p(1)
    raw_refused(fx, L.lm_index_genome_seqs(gi.h, None, C.byref(sp)), ARG, "lm_index_genome_seqs: genome_id is NULL")
    assert sp.value is None
    for a, b in ((gi.subseq(regions, 3, 3), sub), (gi.subseq_rows(rows), by_rows), (gi.genome_seqs("SB"), whole)):
        assert a.seqs == b.seqs and [d["status"] for d in a.info] == [d["status"] for d in b.info] and a.blob == b.blob


def test_a_search_follows_the_refusals(fx):
    """the handle of all the calls above still searches: nothing of a refusal stays with it"""
    gi, gs = fx["gi"], fx["gs"]
    rows, _ = gi.search([gs[3][1][0][1][500:1700]])
    assert rows and rows[0]["genome_id"] == b"SC"
