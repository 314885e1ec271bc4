"""GPU parity of the search flags away from their defaults: HIP path (C-ABI) vs oracle, row for row, for every flag that
reaches the device - seeding (-p, -P), chaining (--seed-max-gap, --seed-max-dist), alignment windows (--align-ext-len) and
pseudo-alignment chaining (--align-band, --align-max-gap, -l, -i) - on their own and together.  Each option set must also
change the rows of the default run, or it would prove nothing.

  search    one batched search per option set on a multi-contig index; gene / read queries plus indel-rich ones (5 %
            substitutions, a 30-90 bp insertion or deletion every ~400 bp), without which the chaining and band flags
            change nothing; CIGAR / qseq / sseq / alignment text byte for byte for two of the sets
  stages    lm_seed_chain_batch against the oracle's seed / clear / Chainer.Chain for the seeding and chaining flags,
            lm_pseudoalign_batch against lmo_cmp_compare (SeqComparator + Chainer2) for the band / gap / -l / -i flags on the
            indel-rich windows of test_pa_chain_far_rounds_cpu.py, whose bands reach the LDS-ring and global-memory rounds
            of pa_chain_dp_reg
  options   lm_index_open refuses every combination the reference refuses (search.go:159-229, lib-index-search.go:483-485)
            with its message, and opens at each boundary value
"""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from test_pa_chain_far_rounds_cpu import cmp_opt, indel_rich, indel_windows, oracle_anchors

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")
ROW_INT = ("batch_genome", "cls", "hsp", "seq_idx", "nseqs", "seq_len", "rc", "aligned_length", "gaps", "qbegin", "qend",
           "tbegin", "tend", "bitscore", "score", "matched_bases")
ROW_F64 = ("qcov_genome", "qcov_hsp", "pident")
LO = "mask_prefix + anchor_prefix"  # placeholder for -p at its lower bound, read from the index

SEED_SETS = {
    "p_lo": dict(min_prefix=LO),
    "p19": dict(min_prefix=19, min_single_prefix=19),
    "p21": dict(min_prefix=21, min_single_prefix=21),
    "p31": dict(min_prefix=31, min_single_prefix=31),
    "P31": dict(min_single_prefix=31),
    "seed_gap5": dict(max_gap=5.0),
    "seed_gap200": dict(max_gap=200.0),
    "seed_dist100": dict(max_distance=100.0),
    "seed_dist10000": dict(max_distance=10000.0),
}
ALIGN_SETS = {
    "band20_gap5": dict(align_band=20, align_max_gap=5),
    "band140": dict(align_band=140),
    "band400": dict(align_band=400),
    "band400_gap100": dict(align_band=400, align_max_gap=100),
    "band1000_gap100": dict(align_band=1000, align_max_gap=100),
    "l200": dict(align_min_match_len=200),
    "i60": dict(align_min_pident=60.0),
    "i99": dict(align_min_pident=99.0),
}
SEARCH_SETS = {
    **SEED_SETS,
    "ext0": dict(ext_len=0, output_seq=1),  # (output_seq: CIGAR / qseq / sseq / alignment text compared too)
    "ext100": dict(ext_len=100),
    "ext5000": dict(ext_len=5000),
    **ALIGN_SETS,
    "band400_gap100": dict(align_band=400, align_max_gap=100, output_seq=1),
    "p19_band400_gap100": dict(min_prefix=19, min_single_prefix=19, align_band=400, align_max_gap=100),
    "p_lo_gap200_dist10000_ext100": dict(min_prefix=LO, max_gap=200.0, max_distance=10000.0, ext_len=100),
    "P31_band140_l200_i60": dict(min_single_prefix=31, align_band=140, align_min_match_len=200, align_min_pident=60.0),
}
# the pseudo-alignment stage: -i reaches Chainer2 only through min_score = -l x -i / 100, below the score of every chain of
# these windows (it filters HSPs by identity later, which the search sets check)
PA_SETS = {k: v for k, v in ALIGN_SETS.items() if "align_min_pident" not in v}


def _la():
    import lexicmap_amd as la
    return la


@pytest.fixture(scope="module")
def mc_index(tmp_path_factory):
    """10 genomes x ~150 kb, 2 families, 3-5 contigs each (as test_gpu_stages_by_option.py); and -p's lower bound"""
    from lexicmap_amd import synth
    d = str(tmp_path_factory.mktemp("optidx") / "mc.lmi")
    genomes = synth.make_genomes(10, 150_000, 2, seed=81, max_div=0.08, contigs=(3, 5))
    O.build_index(d, genomes, O.default_build_opt(chunks=3))
    gi = _la().Index(d)
    info = gi.info()
    gi.close()
    return d, genomes, info["mask_prefix"] + info["anchor_prefix"]


@pytest.fixture(scope="module")
def query_set(mc_index):
    """gene / read queries, two unmutated genome pieces (rows that pass -i 99), 10 indel-rich 4-kb pieces of the genomes and
    the reverse complements of three of them"""
    from lexicmap_amd import synth
    _, genomes, _ = mc_index
    qs = synth.make_gene_queries(genomes, 10, seed=83, len_range=(400, 1800), max_div=0.10)
    qs += synth.make_reads(genomes, 2, seed=84, len_range=(3000, 9000))
    rng = np.random.default_rng(86)
    for i in range(2):
        gid, contigs = genomes[3 + i]
        cid, s = max(contigs, key=lambda c: len(c[1]))
        st = int(rng.integers(0, len(s) - 1500))
        qs.append(("exact%d_%s" % (i, gid), s[st:st + 1500] if i == 0 else s[st:st + 1500].translate(COMP)[::-1]))
    for i in range(10):
        gid, contigs = genomes[int(rng.integers(0, len(genomes)))]
        cid, s = max(contigs, key=lambda c: len(c[1]))
        st = int(rng.integers(0, len(s) - 4000))
        q = indel_rich(rng, np.frombuffer(s[st:st + 4000], dtype=np.uint8)).tobytes()
        qs.append(("indel%d_%s" % (i, gid), q))
        if i < 3:
            qs.append(("indel%d_rc_%s" % (i, gid), q.translate(COMP)[::-1]))
    return [q[0] for q in qs], [q[1] for q in qs]


def _resolve(kw, lo):
    return {k: (lo if v == LO else v) for k, v in kw.items()}


def _oracle_rows(d, kw, seqs):
    oi = O.Index(d, O.default_search_opt(**kw))
    out = [oi.search(s) for s in seqs]
    oi.close()
    return out


def _key(rows):
    return [[tuple(r[f] for f in ROW_INT + ROW_F64) for r in rs] for rs, _ in rows]


@pytest.fixture(scope="module")
def default_rows(mc_index, query_set):
    d, _, _ = mc_index
    return _oracle_rows(d, {}, query_set[1])


@pytest.mark.parametrize("name", list(SEARCH_SETS))
def test_search_rows_equal_the_oracle(mc_index, query_set, default_rows, name):
    la = _la()
    d, _, lo = mc_index
    names, seqs = query_set
    kw = _resolve(SEARCH_SETS[name], lo)
    exp_all = _oracle_rows(d, kw, seqs)
    gi = la.Index(d, la.api.default_options(**kw))
    try:
        rows, _ = gi.search(seqs)
    finally:
        gi.close()
    by_q = {}
    for r in rows:
        by_q.setdefault(r["query"], []).append(r)
    nrows = 0
    for qi, (exp, st) in enumerate(exp_all):
        got = by_q.get(qi, [])
        label = (name, names[qi])
        assert len(exp) == len(got), (label, len(exp), len(got))
        for e, g in zip(exp, got):
            for f in ROW_INT + ROW_F64:
                assert e[f] == g[f], (label, f, e[f], g[f])
            assert g["evalue"] == pytest.approx(e["evalue"], rel=1e-9, abs=0)
            assert e["genome_id"] == g["genome_id"] and e["seq_id"] == g["seq_id"]
            assert g["hits"] == st["ngenomes"], label
            if kw.get("output_seq"):
                assert (e["cigar"], e["qseq"], e["tseq"], e["align"]) == (g["cigar"], g["qseq"], g["sseq"], g["align"]), label
                assert e["cigar"]
        nrows += len(exp)
    assert nrows >= (3 if name == "i99" else 100), (name, nrows)
    # the option set matters: the rows are not those of the default run
    assert _key(exp_all) != _key(default_rows), name


def _oracle_pairs(oi, seq, kw):
    """oracle per genome: raw anchors (clear order), cleared anchors, score, chains - test_gpu_parity._oracle_pairs with the
    chaining parameters of the option set (lib-index-search.go:742, :1057)"""
    L = O.lib()
    M = oi.nmasks
    if len(seq) < 31:
        return {}
    ok = (C.c_uint64 * M)()
    ooff, olocs = C.POINTER(C.c_int)(), C.POINTER(C.c_int)()
    L.lmo_stage_mask(oi.h, seq, len(seq), ok, C.byref(ooff), C.byref(olocs))
    anc = C.POINTER(O.Anchor)()
    na = L.lmo_stage_anchors(oi.h, ok, ooff, olocs, C.byref(anc))
    max_gap = float(kw.get("max_gap", 50.0))
    max_dist = float(kw.get("max_distance", 1000.0))
    min_score = L.lmo_seed_weight(float(kw.get("min_single_prefix", 17)))
    tup = lambda s: (s.qbegin, s.tbegin, s.len, s.qrc, s.trc)
    out = {}
    i = 0
    while i < na:
        j = i
        while j < na and anc[j].genome == anc[i].genome:
            j += 1
        n = j - i
        subs = (O.Sub * n)()
        for t in range(n):
            subs[t] = anc[i + t].sub
        raw = [tup(subs[t]) for t in range(n)]
        nn = L.lmo_clear_subs(subs, n, 31) if n > 1 else n
        cleared = [tup(subs[t]) for t in range(nn)]
        coff, cidx, nch = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.c_int()
        sc = L.lmo_chainer(subs, nn, max_gap, min_score, max_dist, 0, C.byref(coff), C.byref(cidx), C.byref(nch))
        chains = [[cidx[x] for x in range(coff[c], coff[c + 1])] for c in range(nch.value)]
        out[anc[i].genome] = dict(raw=raw, cleared=cleared, score=np.float32(sc).tobytes(), chains=chains)
        L.free(coff)
        L.free(cidx)
        i = j
    L.free(anc)
    L.free(ooff)
    L.free(olocs)
    return out


def _all_oracle_pairs(d, kw, seqs):
    oi = O.Index(d, O.default_search_opt(**kw))
    out = [_oracle_pairs(oi, s, kw) for s in seqs]
    oi.close()
    return out


@pytest.fixture(scope="module")
def default_pairs(mc_index, query_set):
    d, _, _ = mc_index
    return _all_oracle_pairs(d, {}, query_set[1])


@pytest.mark.parametrize("name", list(SEED_SETS))
def test_seed_and_chain_stages_equal_the_oracle(mc_index, query_set, default_pairs, name):
    """prefix + suffix lookup, anchor assembly, ClearSubstrPairs and Chainer.Chain (raw, cleared, float32 score, chains)"""
    la = _la()
    d, _, lo = mc_index
    names, seqs = query_set
    kw = _resolve(SEED_SETS[name], lo)
    exp_all = _all_oracle_pairs(d, kw, seqs)
    gi = la.Index(d, la.api.default_options(**kw))
    try:
        pairs = gi.seed_chain(seqs)
    finally:
        gi.close()
    by_q = {}
    for p in pairs:
        by_q.setdefault(p["query"], {})[p["genome"]] = p
    total = 0
    for qi, exp in enumerate(exp_all):
        got = by_q.get(qi, {})
        assert sorted(exp) == sorted(got), (name, names[qi])
        for g, e in exp.items():
            p = got[g]
            label = (name, names[qi], g)
            assert p["raw"] == e["raw"], label
            assert p["cleared"] == e["cleared"], label
            assert np.float32(p["score"]).tobytes() == e["score"], label
            assert p["chains"] == e["chains"], label
            total += len(e["raw"])
    assert total > 1000
    assert exp_all != default_pairs, name


def _oracle_chains(queries, problems, kw):
    return [ch for ch, _ in oracle_anchors(queries, problems, cmp_opt(**kw))]


@pytest.mark.parametrize("name", list(PA_SETS))
def test_pseudoalign_stage_equals_the_oracle(mc_index, name):
    """SeqComparator.Compare + Chainer2 (k_pa_chain_wave: pa_chain_dp_reg and its far rounds, pa_chain_backtrack_wave) on
    windows whose bands outgrow the 64 registers and the LDS ring (the windows come from the caller, the options from the
    handle)"""
    la = _la()
    d, _, _ = mc_index
    queries, problems = indel_windows()
    kw = PA_SETS[name]
    exp = _oracle_chains(queries, problems, kw)
    gi = la.Index(d, la.api.default_options(**kw))
    try:
        got = gi.pseudoalign(queries, problems)
    finally:
        gi.close()
    assert len(got) == len(problems)
    nchains = 0
    for pi, (e, g) in enumerate(zip(exp, got)):
        g = [(c["qbegin"], c["qend"], c["tbegin"], c["tend"], c["nanchors"], c["matched_bases"], c["aligned_bases_q"],
              c["aligned_bases_t"], c["pident"]) for c in g]
        assert g == e, (name, pi)
        nchains += len(e)
    assert nchains >= len(problems)
    assert exp != _oracle_chains(queries, problems, {}), name


def _open_error(d, **kw):
    la = _la()
    with pytest.raises(RuntimeError) as ei:
        la.Index(d, la.api.default_options(**kw))
    return str(ei.value)


def test_index_open_checks_the_options(mc_index):
    la = _la()
    d, _, lo = mc_index
    p_range = "should be in the range of [5, 32]"
    p_k = "MinPrefix (%d) should be in the range of [%d, 31]"
    P_msg = "-P/--seed-min-single-prefix should be >= -p and <= 32"
    refused = [
        (dict(min_prefix=4), p_range),
        (dict(min_prefix=33, min_single_prefix=33, align_min_match_len=50), p_range),
        (dict(min_prefix=32, min_single_prefix=32), p_k % (32, lo)),
        (dict(min_prefix=lo - 1), p_k % (lo - 1, lo)),
        (dict(min_prefix=19, min_single_prefix=18), P_msg),
        (dict(min_single_prefix=33), P_msg),
        (dict(align_band=19, align_max_gap=20), "--align-band should be >= --align-max-gap"),
        (dict(align_min_match_len=16), "-l/--align-min-match-len should be >= -P/--seed-min-single-prefix"),
        (dict(align_min_pident=59.9), "-i/--align-min-match-pident should be in range of [60, 100]"),
        (dict(align_min_pident=100.1), "-i/--align-min-match-pident should be in range of [60, 100]"),
        (dict(max_gap=0.0), "seed-max-gap / seed-max-dist / align-ext-len out of range"),
        (dict(max_distance=0.0), "seed-max-gap / seed-max-dist / align-ext-len out of range"),
        (dict(ext_len=-1), "seed-max-gap / seed-max-dist / align-ext-len out of range"),
    ]
    for kw, msg in refused:
        err = _open_error(d, **kw)
        assert msg in err, (kw, err)
    accepted = [dict(min_prefix=lo), dict(min_prefix=31, min_single_prefix=31), dict(min_single_prefix=32),
                dict(align_band=20, align_max_gap=20), dict(align_min_match_len=17), dict(align_min_pident=60.0),
                dict(align_min_pident=100.0), dict(ext_len=0)]
    for kw in accepted:
        gi = la.Index(d, la.api.default_options(**kw))
        gi.close()
