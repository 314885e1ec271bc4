"""Genome residency (lm_residency, DESIGN.md "Residency of the 2-bit genomes"): the 2-bit genomes of a handle in HBM, in
pinned host memory, or split between the two.  Wherever a genome lives the rows are the same: the long-read fixture of
test_gpu_longreads.py (windows of tens of kb, the wide WFA passes, chunks and rounds) searched under every placement against
the CPU oracle and against a default handle; the staging kernel k_stage_genome_bits must run exactly when a host-resident
genome is touched.
"""
import hashlib
import os

import numpy as np
import pytest

import oracle as O
from test_gpu_longreads import _cmp

pytestmark = pytest.mark.gpu


def _la():
    import lexicmap_amd as la
    return la


def _res(genomes, budget=0):
    from lexicmap_amd import api
    return api.Residency(genomes, budget)


@pytest.fixture(scope="module")
def res_index(tmp_path_factory):
    """8 genomes x ~400 kb in 2 families (<= 6 % divergence), 1-2 contigs"""
    from lexicmap_amd import synth
    d = str(tmp_path_factory.mktemp("residx") / "res.lmi")
    genomes = synth.make_genomes(8, 400_000, 2, seed=21, max_div=0.06, contigs=(1, 2))
    O.build_index(d, genomes, O.default_build_opt(chunks=4))
    return d, genomes


@pytest.fixture(scope="module")
def res_queries(res_index):
    """reads of 5-50 kb from several genomes, one at each end of the range, and a reverse-strand 120-kb query"""
    from lexicmap_amd import synth
    _, genomes = res_index
    qs = synth.make_reads(genomes, 5, seed=31, len_range=(5000, 50000))
    rng = np.random.default_rng(32)
    gid, contigs = genomes[3]
    s = np.frombuffer(max(contigs, key=lambda c: len(c[1]))[1], dtype=np.uint8)
    qs.append(("r50k", synth.mutate(rng, s[1000:51000], sub=0.02, ins=0.02, dele=0.03).tobytes()))
    qs.append(("r5k", synth.mutate(rng, s[60000:65000], sub=0.02, ins=0.02, dele=0.03).tobytes()))
    region = s[100000:220000]
    rot = np.concatenate([region[70000:], region[:70000]])
    rot = synth.mutate(rng, rot, sub=0.01, ins=0.002, dele=0.002)
    qs.append(("circ120k_rc", rot.tobytes().translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]))
    return qs


@pytest.fixture(scope="module")
def default_rows(res_index, res_queries):
    """rows, statistics, info and residency of a default handle (plain lm_index_open), and the same with output_seq"""
    la = _la()
    d, _ = res_index
    seqs = [q[1] for q in res_queries]
    gi = la.Index(d)
    gi.profile(True)
    rows, st = gi.search(seqs)
    prof = {p["name"]: p for p in gi.profile_get()}
    info, res = gi.info(), gi.residency()
    gi.close()
    gs = la.Index(d, la.api.default_options(output_seq=1))
    rows_seq, _ = gs.search(seqs)
    gs.close()
    return dict(rows=rows, stats=st, prof=prof, info=info, res=res, rows_seq=rows_seq)


def _stage(gi):
    for p in gi.profile_get():
        if p["name"] == "k_stage_genome_bits":
            return p
    return dict(launches=0, bytes=0, total_ms=0.0)


def _split_is_hit(rows, host_keys, device_keys):
    """the batch's rows touch genomes on both sides of a placement split"""
    hit = {r["batch_genome"] for r in rows}
    assert hit & set(host_keys), (sorted(hit), host_keys)
    assert hit & set(device_keys), (sorted(hit), device_keys)


def test_default_handle_has_everything_on_the_device(default_rows):
    r = default_rows["res"]
    assert r["stage_bytes"] == 0   # (after a search: a handle without host-resident genomes stages nothing)
    assert r["genomes_device"] == 8 and r["genomes_host"] == 0 and r["genome_bytes_host"] == 0
    assert r["genome_bytes_device"] > 8 * 100_000
    assert default_rows["prof"].get("k_stage_genome_bits", dict(launches=0))["launches"] == 0


def test_all_genomes_on_host_equal_the_oracle_and_the_default_handle(res_index, res_queries, default_rows):
    la = _la()
    d, _ = res_index
    seqs = [q[1] for q in res_queries]
    gi = la.Index(d, residency=_res(la.api.GENOMES_HOST))
    r = gi.residency()
    assert r["stage_bytes"] == 0   # nothing searched yet
    assert r["genomes_device"] == 0 and r["genomes_host"] == 8 and r["genome_bytes_device"] == 0
    assert r["genome_bytes_host"] >= default_rows["res"]["genome_bytes_device"] - 8 * 16
    # hbm_bytes counts device bytes only
    assert default_rows["info"]["hbm_bytes"] - gi.info()["hbm_bytes"] >= default_rows["res"]["genome_bytes_device"]
    gi.profile(True)
    rows, stats = gi.search(seqs)
    sp = _stage(gi)
    # the staging buffer of the last chunk stays with the handle until its next search re-cuts the scratch
    assert gi.residency()["stage_bytes"] > 0
    gi.close()
    assert sp["launches"] > 0 and sp["bytes"] > 0
    assert rows == default_rows["rows"]
    oi = O.Index(d)
    by_q = {}
    for row in rows:
        by_q.setdefault(row["query"], []).append(row)
    nrows, longest = 0, 0
    for qi, s in enumerate(seqs):
        exp, st = oi.search(s)
        got = by_q.get(qi, [])
        _cmp(exp, got, res_queries[qi][0])
        for g in got:
            assert g["hits"] == st["ngenomes"]
            longest = max(longest, g["aligned_length"])
        nrows += len(exp)
    oi.close()
    assert nrows >= 20 and longest > 40000   # the wide windows really ran
    assert stats["rows"] == nrows
    # -a: cigar / qseq / sseq / align strings included
    gs = la.Index(d, la.api.default_options(output_seq=1), residency=_res(la.api.GENOMES_HOST))
    rows_seq, _ = gs.search(seqs)
    gs.close()
    assert rows_seq == default_rows["rows_seq"]
    assert any(r.get("cigar") for r in rows_seq)


def test_mixed_placement_stages_only_the_host_side(res_index, res_queries, default_rows):
    la = _la()
    d, _ = res_index
    seqs = [q[1] for q in res_queries]
    total = default_rows["res"]["genome_bytes_device"]
    budget = total // 2
    gh = la.Index(d, residency=_res(la.api.GENOMES_HOST))
    gh.profile(True)
    gh.search(seqs)
    host_bytes = _stage(gh)["bytes"]
    gh.close()
    gi = la.Index(d, residency=_res(la.api.GENOMES_AUTO, budget))
    r = gi.residency()
    assert r["genomes_device"] > 0 and r["genomes_host"] > 0 and r["genomes_device"] + r["genomes_host"] == 8
    assert r["genome_bytes_device"] <= budget
    gi.profile(True)
    rows, _ = gi.search(seqs)
    sp = _stage(gi)
    gi.close()
    assert rows == default_rows["rows"]
    nd = r["genomes_device"]   # a prefix of the local order stays on the device; one batch: key = local number
    _split_is_hit(rows, host_keys=list(range(nd, 8)), device_keys=list(range(nd)))
    assert sp["launches"] > 0 and 0 < sp["bytes"] < host_bytes
    assert default_rows["prof"].get("k_stage_genome_bits", dict(launches=0))["launches"] == 0


def test_explicit_device_and_null_residency(res_index, res_queries, default_rows):
    la = _la()
    d, _ = res_index
    seqs = [q[1] for q in res_queries]
    for res in (_res(la.api.GENOMES_DEVICE), _res(la.api.GENOMES_AUTO, 0), None):
        gi = la.Index(d, residency=res)
        assert gi.residency()["genomes_host"] == 0 and gi.residency()["genomes_device"] == 8
        gi.profile(True)
        rows, _ = gi.search(seqs)
        assert _stage(gi)["launches"] == 0
        assert gi.info()["hbm_bytes"] == default_rows["info"]["hbm_bytes"]
        gi.close()
        assert rows == default_rows["rows"]


@pytest.mark.parametrize("two_lanes", [True, False])
def test_chunks_and_rounds_under_host_placement(res_index, res_queries, monkeypatch, two_lanes):
    """several pseudo-alignment chunks per part, a round every few HSPs, several parts: the staged ranges of a chunk must
    live until its windows are extracted.  The reads up to 50 kb only: LM_MAX_PART_KMERS=60000 is less than the 120-kb
    query alone, which the library refuses on any handle (as test_gpu_longreads.py leaves it out of its parts test)."""
    la = _la()
    d, _ = res_index
    seqs = [q[1] for q in res_queries if len(q[1]) <= 59000]
    assert len(seqs) == len(res_queries) - 1
    g0 = la.Index(d, la.api.default_options(output_seq=1))   # default placement, single round
    base, _ = g0.search(seqs)
    g0.close()
    assert len(base) >= 20 and max(r["aligned_length"] for r in base) > 40000
    g1 = la.Index(d, la.api.default_options(output_seq=1), residency=_res(la.api.GENOMES_HOST))   # host placement, nothing forced
    g1.profile(True)
    plain, _ = g1.search(seqs)
    plain_launches = _stage(g1)["launches"]
    g1.close()
    assert plain == base and plain_launches >= 1
    if not two_lanes:
        monkeypatch.setenv("LM_TWO_LANES", "0")
    for k, v in (("LM_DEBUG_MAX_WINDOW_BYTES", "150000"), ("LM_DEBUG_ROUND_HSPS", "4"), ("LM_DEBUG_MIN_ROUND_HSPS", "1"),
                 ("LM_MAX_PART_KMERS", "60000")):
        monkeypatch.setenv(k, v)
    gi = la.Index(d, la.api.default_options(output_seq=1), residency=_res(la.api.GENOMES_HOST))
    gi.profile(True)
    rows, _ = gi.search(seqs)
    sp = _stage(gi)
    gi.close()
    # really in chunks: one staging launch per pseudo-alignment chunk, and the forced run cuts the batch into several parts
    # with at least one chunk each, where the plain run above had all its windows in the chunk(s) of one part
    assert sp["launches"] > plain_launches
    assert rows == base


def test_options_that_cut_the_genome_set(res_index, res_queries):
    la = _la()
    d, _ = res_index
    seqs = [q[1] for q in res_queries]
    # -n 2
    opt = dict(top_n_genomes=2)
    g0 = la.Index(d, la.api.default_options(**opt))
    base, _ = g0.search(seqs)
    full_bytes = g0.residency()["genome_bytes_device"]
    g0.close()
    g1 = la.Index(d, la.api.default_options(**opt), residency=_res(la.api.GENOMES_HOST))
    rows, _ = g1.search(seqs)
    g1.close()
    assert rows == base and len(base) > 0
    # a genome filter that keeps only host-resident genomes of a mixed handle
    g0 = la.Index(d)
    g1 = la.Index(d, residency=_res(la.api.GENOMES_AUTO, full_bytes // 2))
    nd = g1.residency()["genomes_device"]
    assert 0 < nd < 8
    keys = list(range(nd, 8))
    g0.set_genome_filter(keys)
    g1.set_genome_filter(keys)
    base, _ = g0.search(seqs)
    g1.profile(True)
    rows, _ = g1.search(seqs)
    assert _stage(g1)["launches"] > 0
    g0.close()
    g1.close()
    assert rows == base and len(base) > 0
    assert {r["batch_genome"] for r in rows} <= set(keys)


def test_two_shards_on_host_merge_to_the_unsharded_rows(res_index, res_queries, default_rows):
    la = _la()
    from lexicmap_amd import merge
    from test_gpu_parity import ROW_F64, ROW_INT
    d, _ = res_index
    seqs = [q[1] for q in res_queries]
    rows_w = default_rows["rows"]
    tb = default_rows["info"]["total_bases"]
    shards = [la.Index(d, la.api.default_options(shard_rank=r, shard_count=2, total_bases_override=tb),
                       residency=_res(la.api.GENOMES_HOST)) for r in range(2)]
    per_rank = []
    for si in shards:
        assert si.residency()["genomes_host"] == 4 and si.residency()["genomes_device"] == 0
        qb = si.upload(seqs)
        arr, _ = si.search_resident_np(qb)
        per_rank.append(arr.copy())
        si.free_batch(qb)
    merged, names = merge.merge_sharded_c(per_rank, shards[0])
    for si in shards:
        si.close()
    assert len(merged) == len(rows_w) >= 20
    for i, w in enumerate(rows_w):
        for f in ROW_INT + ROW_F64 + ["evalue", "hits", "query"]:
            assert merged[f][i] == w[f], (i, f)
        assert names[i] == (w["genome_id"], w["seq_id"]), i


def _tree_hashes(root):
    out = {}
    for sub in ("genomes", "seeds"):
        for dp, _, files in os.walk(os.path.join(root, sub)):
            for f in files:
                p = os.path.join(dp, f)
                with open(p, "rb") as fh:
                    out[os.path.relpath(p, root)] = hashlib.sha256(fh.read()).hexdigest()
    return out


def test_fetch_and_save_read_a_genome_where_it_lives(res_index, tmp_path):
    la = _la()
    d, _ = res_index
    g0 = la.Index(d)
    g1 = la.Index(d, residency=_res(la.api.GENOMES_HOST))
    glen = g0.info()["genome_bases"]
    assert glen == g1.info()["genome_bases"]
    for g in (0, 3, 7):
        # the length of genome g, from its last fetchable base
        lo, hi = 1, 2_000_000
        while lo < hi:   # largest n with fetch(g, n - 1, 1) valid
            mid = (lo + hi + 1) // 2
            try:
                g0.fetch(g, mid - 1, 1)
                lo = mid
            except RuntimeError:
                hi = mid - 1
        n = lo
        for start, ln in ((0, 100), (3, 77), (61, 70), (n - 100, 100), (n - 67, 67), (n - 130, 129), (0, n)):
            assert g1.fetch(g, start, ln) == g0.fetch(g, start, ln), (g, start, ln)
    a, b = str(tmp_path / "a.lmi"), str(tmp_path / "b.lmi")
    g0.save(a, 4)
    g1.save(b, 4)
    g0.close()
    g1.close()
    ha, hb = _tree_hashes(a), _tree_hashes(b)
    assert ha == hb and len(ha) >= 4


def test_synthetic_builder_moves_the_genomes_to_the_host():
    la = _la()
    kw = dict(seed=77, max_div=0.08, masks=5000)
    g0 = la.Index.synthetic(24, 120_000, 3, residency=None, **kw)
    g1 = la.Index.synthetic(24, 120_000, 3, residency=_res(la.api.GENOMES_HOST), **kw)
    r0, r1 = g0.residency(), g1.residency()
    assert r0["genomes_device"] == 24 and r0["genomes_host"] == 0
    assert r1["genomes_host"] == 24 and r1["genomes_device"] == 0 and r1["genome_bytes_device"] == 0
    assert g0.info()["hbm_bytes"] - g1.info()["hbm_bytes"] >= r0["genome_bytes_device"]
    rng = np.random.default_rng(5)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs = []
    for i in range(12):   # queries derived from the set itself, every other one reverse strand
        g, st, ln = int(rng.integers(0, 24)), int(rng.integers(0, 100_000)), int(rng.integers(600, 9000))
        s = g0.fetch(g, st, ln)
        assert s == g1.fetch(g, st, ln)
        seqs.append(s.translate(comp)[::-1] if i % 2 else s)
    base, _ = g0.search(seqs)
    g1.profile(True)
    rows, _ = g1.search(seqs)
    assert _stage(g1)["launches"] > 0
    g0.close()
    g1.close()
    assert rows == base and len(base) >= 12


def test_environment_override_and_explicit_argument(res_index, res_queries, default_rows, monkeypatch):
    la = _la()
    d, _ = res_index
    seqs = [q[1] for q in res_queries]
    monkeypatch.setenv("LM_GENOME_PLACEMENT", "host")
    gi = la.Index(d)
    ge = la.Index(d, residency=_res(la.api.GENOMES_DEVICE))   # an explicit argument wins
    monkeypatch.delenv("LM_GENOME_PLACEMENT")
    assert gi.residency()["genomes_host"] == 8
    assert ge.residency()["genomes_host"] == 0 and ge.residency()["genomes_device"] == 8
    rows, _ = gi.search(seqs)
    gi.close()
    ge.close()
    assert rows == default_rows["rows"]
    monkeypatch.setenv("LM_GENOME_HBM_MB", "1")   # a byte budget from the environment: the device share stays within it
    gi = la.Index(d)
    monkeypatch.delenv("LM_GENOME_HBM_MB")
    r = gi.residency()
    gi.close()
    # the fixture's store (3.2 Mb of genomes: ~0.8 MB of 2-bit bytes) is within 1 MB: the budget is honoured by keeping all of it
    assert default_rows["res"]["genome_bytes_device"] <= 1 << 20
    assert r["genomes_device"] == 8 and r["genomes_host"] == 0
    assert r["genome_bytes_device"] == default_rows["res"]["genome_bytes_device"]
    monkeypatch.setenv("LM_GENOME_HBM_MB", "0")   # not a budget: refused with a message, not read as "derive" or "nothing"
    with pytest.raises(RuntimeError, match="LM_GENOME_HBM_MB"):
        la.Index(d)
    monkeypatch.delenv("LM_GENOME_HBM_MB")


def test_unknown_placement_is_refused_with_a_message(res_index):
    import ctypes as C
    la = _la()
    d, _ = res_index
    L = la.lib()
    L.lm_last_error.restype = C.c_char_p
    h = C.c_void_p()
    opt = la.api.default_options()
    bad = la.api.Residency(7, 0)
    st = L.lm_index_open_ex(d.encode(), C.byref(opt), C.byref(bad), 0, C.byref(h))
    assert st in (3, 7) and not h.value   # LM_ERR_OPTION (as the option checks) or LM_ERR_ARG
    assert b"genomes" in L.lm_last_error(None)
    sp = la.api.SynthSpec(31, 5000, 1, 4, 50_000, 2, 0.05, 3, 100, 50)
    st = L.lm_index_build_synthetic_ex(C.byref(sp), C.byref(opt), C.byref(bad), 0, C.byref(h))
    assert st in (3, 7) and not h.value
    assert L.lm_last_error(None)
    with pytest.raises(RuntimeError):
        la.Index(d, residency=bad)
