"""k_pa_search does not emit pseudo-alignment anchors that are nested in the anchor of the neighbouring window position
(lm_pa_anchor_nested): ClearSubstrPairs would drop them.  With the rule off (LM_PA_DROP_NESTED=0, read by
lm_tuning_reload) and on, one handle must give the same rows in every column and the same number of chains from fewer
anchors - on a handle with the genomes in HBM, on one with host-resident genomes (the other instantiation of the kernel),
with the two-key anchor layout and through the re-run after an overflow of the anchor buffer.  Caller-supplied ASCII windows
(lm_pseudoalign_batch) keep every anchor."""
import pytest

import oracle as O

pytestmark = pytest.mark.gpu


def _la():
    import lexicmap_amd as la
    return la


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """24 genomes x ~120 kb in 4 families; reads of 2-8 kb and the reverse complements of two of them"""
    from lexicmap_amd import synth
    d = str(tmp_path_factory.mktemp("panested") / "small.lmi")
    genomes = synth.make_genomes(24, 120000, 4, seed=11, max_div=0.12, contigs=(1, 4), with_n=True)
    O.build_index(d, genomes, O.default_build_opt(chunks=4))
    reads = [q[1] for q in synth.make_reads(genomes, 6, seed=6, len_range=(2000, 8000))]
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    reads += [r.translate(comp)[::-1] for r in reads[:2]]
    return d, genomes, reads


def _off_and_on(gi, seqs, monkeypatch):
    monkeypatch.setenv("LM_PA_DROP_NESTED", "0")
    gi.tuning_reload()
    off = gi.search(seqs)
    monkeypatch.setenv("LM_PA_DROP_NESTED", "1")
    gi.tuning_reload()
    on = gi.search(seqs)
    monkeypatch.delenv("LM_PA_DROP_NESTED")
    gi.tuning_reload()
    return off, on


def _same_rows_fewer_anchors(off, on):
    (rows0, st0), (rows1, st1) = off, on
    assert len(rows0) == len(rows1) and len(rows0) > 20
    for a, b in zip(rows0, rows1):
        assert a == b
    assert {r["rc"] for r in rows0} == {0, 1}      # windows of both orientations
    assert st0["rows"] == st1["rows"] and st0["chains"] == st1["chains"] and st0["chains"] > 0
    print("pa_anchors: %d with every anchor, %d without the nested ones" % (st0["pa_anchors"], st1["pa_anchors"]))
    assert 0 < st1["pa_anchors"] < st0["pa_anchors"]


def test_rows_and_chains_are_equal_and_anchors_fewer(fx, monkeypatch):
    la = _la()
    d, _, reads = fx
    gi = la.Index(d)
    off, on = _off_and_on(gi, reads, monkeypatch)
    default = gi.search(reads)       # the rule is on by default
    gi.close()
    _same_rows_fewer_anchors(off, on)
    assert default[0] == on[0] and default[1]["pa_anchors"] == on[1]["pa_anchors"]


def test_host_resident_genomes(fx, monkeypatch):
    la = _la()
    d, _, reads = fx
    gi = la.Index(d, residency=la.api.Residency(la.api.GENOMES_HOST, 0))
    assert gi.residency()["genomes_host"] == 24
    off, on = _off_and_on(gi, reads, monkeypatch)
    gi.close()
    _same_rows_fewer_anchors(off, on)


def test_pair_keys(fx, monkeypatch):
    la = _la()
    d, _, reads = fx
    gi = la.Index(d)
    base = gi.search(reads)
    monkeypatch.setenv("LM_DEBUG_PA_WIDE_KEYS", "1")
    off, on = _off_and_on(gi, reads, monkeypatch)
    monkeypatch.delenv("LM_DEBUG_PA_WIDE_KEYS")
    gi.close()
    _same_rows_fewer_anchors(off, on)
    assert on[0] == base[0] and on[1]["pa_anchors"] == base[1]["pa_anchors"]


def test_anchor_buffer_overflow_rerun(fx, monkeypatch):
    la = _la()
    d, _, reads = fx
    gi = la.Index(d)
    base = gi.search(reads)
    monkeypatch.setenv("LM_DEBUG_PA_CAP", "1000")
    off, on = _off_and_on(gi, reads, monkeypatch)
    monkeypatch.delenv("LM_DEBUG_PA_CAP")
    gi.close()
    _same_rows_fewer_anchors(off, on)
    assert on[0] == base[0] and on[1]["pa_anchors"] == base[1]["pa_anchors"]


def test_caller_supplied_windows_keep_every_anchor(fx, monkeypatch):
    """lm_pseudoalign_batch: ASCII windows have no packed genome behind them, the rule does not apply and the chains do not
    depend on the switch"""
    la = _la()
    d, _, reads = fx
    gi = la.Index(d)
    problems = []
    for qi in range(3):   # a stretch of the read with a substitution every 47 bases (runs shorter than 2 K) between foreign flanks
        other = reads[(qi + 1) % 3]
        mid = bytearray(reads[qi][200:1800])
        for at in range(23, len(mid), 47):
            mid[at] = {65: 67, 67: 71, 71: 84, 84: 65}.get(mid[at], 67)
        problems.append((qi, 0, len(reads[qi]) - 1, other[:300] + bytes(mid) + other[300:500]))
    qs = reads[:3]
    monkeypatch.setenv("LM_PA_DROP_NESTED", "0")
    gi.tuning_reload()
    off = gi.pseudoalign(qs, problems)
    monkeypatch.setenv("LM_PA_DROP_NESTED", "1")
    gi.tuning_reload()
    on = gi.pseudoalign(qs, problems)
    monkeypatch.delenv("LM_PA_DROP_NESTED")
    gi.close()
    assert off == on and sum(len(c) for c in on) > 0
