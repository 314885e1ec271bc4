"""The pseudo-alignment anchors of k_pa_filter + k_pa_search on the named edges of tests/pa_cases.py, held to the plain model of
tests/pa_model.py.  The windows are ranges of the resident 2-bit genomes and go through lm_pseudoalign_regions, i.e. through the
kernels a search runs (rolling / strided fast path, the partial-prefix rule in LDS, the pending list of long queries, the
nested-anchor rule, the per-task sources of a handle with host-resident genomes); the same windows as ASCII text go through
lm_pseudoalign_batch_ex.  The emitted anchor lists themselves are compared, exactly:
  * rule off (LM_PA_DROP_NESTED=0): emitted == the model's raw list, per problem, and in the ClearSubstrPairs order;
  * default tuning: emitted is a sub-multiset of raw, ClearSubstrPairs(emitted) == ClearSubstrPairs(raw), fewer are emitted, and the
    chains equal lmo_cmp_compare on the window text;
  * the same under LM_PA_FILTER_ROLL=0, LM_DEBUG_PA_WIDE_KEYS=1, a small LM_DEBUG_PA_CAP and on host-resident genomes
    (the by-group segment layout, lm_tune::pa_seg_by_group, has no environment switch: the calls with one short query run the
    per-wavefront layout, the others the by-group one);
  * the windows a search opens, rebuilt from lm_seed_chain_batch, give through the seam the search's own window and anchor counts."""
import collections
import ctypes as C

import pytest

import oracle as O
import pa_cases as PC
import pa_model as M

pytestmark = pytest.mark.gpu
K = 31


def _la():
    import lexicmap_amd as la
    return la


@pytest.fixture(scope="module")
def fx():
    la = _la()
    f = PC.build()
    bo = la.BuildOpt.default(masks=1024)
    f["dev"] = la.Index.from_genomes(f["genomes"], bo)
    f["host"] = la.Index.from_genomes(f["genomes"], bo, residency=la.api.Residency(la.api.GENOMES_HOST, 0))
    assert f["host"].residency()["genomes_host"] == len(f["genomes"]) and f["dev"].residency()["genomes_host"] == 0
    # the model sees the genomes as the library returns them; they are the input under the store's base table
    f["fetched"] = [f["dev"].fetch(g, 0, len(gs[1][0][1])) for g, gs in enumerate(f["genomes"])]
    for g, gs in enumerate(f["genomes"]):
        assert f["fetched"][g] == gs[1][0][1].translate(PC.STORE_TABLE), gs[0]
        assert f["host"].fetch(g, 0, len(gs[1][0][1])) == f["fetched"][g]
    assert any(f["fetched"][g] != gs[1][0][1] for g, gs in enumerate(f["genomes"]))   # (a genome holds non-ACGT bytes)
    f["res"] = PC.run_models(f)
    yield f
    f["dev"].close()
    f["host"].close()
    for q in f["qindex"].values():
        q.close()


def _call(fx, gi, call, packed=True):
    """one library call for the cases of `call`, with only the queries they use: (case numbers, chains, anchors)"""
    idx = fx["calls"][call]
    cases = [fx["cases"][i] for i in idx]
    used = sorted({c.q for c in cases})
    qmap = {q: n for n, q in enumerate(used)}
    queries = [fx["queries"][q] for q in used]
    if packed:
        chains, anchors = gi.pseudoalign_regions(queries, [(qmap[c.q], c.qbegin, c.qend, c.g, c.tbegin, c.wlen, c.rc) for c in cases])
    else:
        chains, anchors = gi.pseudoalign_anchors(queries, [(qmap[c.q], c.qbegin, c.qend, fx["res"][i].text) for i, c in zip(idx, cases)])
    return idx, chains, anchors


def _assert_raw(fx, idx, anchors, label):
    n = 0
    for i, got in zip(idx, anchors):
        r, c = fx["res"][i], fx["cases"][i]
        if sorted(got) != sorted(r.raw):
            miss, extra = collections.Counter(r.raw) - collections.Counter(got), collections.Counter(got) - collections.Counter(r.raw)
            raise AssertionError("%s, case %s: %d emitted, %d in the model; missing %s, not in the model %s" % (
                label, c.name, len(got), len(r.raw), sorted(miss.elements())[:6], sorted(extra.elements())[:6]))
        keys = [M.sort_key(a) for a in got]
        assert all(keys[j] <= keys[j + 1] for j in range(len(keys) - 1)), "%s, case %s: emitted order" % (label, c.name)
        n += len(got)
    return n


CALLS = ("main", "n63", "n64", "n65", "n129", "three_queries")
# the tandem repeats ("many": > 10^5 anchors per window, which k_pa_chain takes ~5 s to chain - the profile of the call says so)
# run once per property: rule off on either handle, rule off through the re-run after an overflow, default tuning


def _rule_off_everywhere(fx, gi, monkeypatch, label, calls=CALLS):
    monkeypatch.setenv("LM_PA_DROP_NESTED", "0")
    gi.tuning_reload()
    try:
        total = 0
        for call in calls:
            idx, _, anchors = _call(fx, gi, call)
            total += _assert_raw(fx, idx, anchors, "%s, call %s" % (label, call))
    finally:
        monkeypatch.delenv("LM_PA_DROP_NESTED")
        gi.tuning_reload()
    return total


@pytest.mark.parametrize("handle", ["dev", "host"])
def test_rule_off_emits_exactly_the_raw_list(fx, monkeypatch, handle):
    fam, tot = PC.check_reached(fx, fx["res"])
    calls = CALLS + ("many",)
    n = _rule_off_everywhere(fx, fx[handle], monkeypatch, handle, calls)
    print("pa edges on the GPU (%s): raw %d, quirk %d, forward %d, reverse %d, multi-match positions %d; %d anchors compared over %d calls" % (
        handle, tot["raw"], tot["quirk"], tot["fwd"], tot["rev"], tot["multi"], n, len(calls)))
    assert n > tot["raw"]


@pytest.mark.parametrize("handle", ["dev", "host"])
@pytest.mark.parametrize("switch", [("LM_PA_FILTER_ROLL", "0"), ("LM_DEBUG_PA_WIDE_KEYS", "1"), ("LM_DEBUG_PA_CAP", "1000")])
def test_rule_off_under_switches(fx, monkeypatch, handle, switch):
    monkeypatch.setenv(*switch)
    try:
        calls = ("main", "n65", "three_queries") + (("many",) if handle == "dev" and switch[0] == "LM_DEBUG_PA_CAP" else ())
        _rule_off_everywhere(fx, fx[handle], monkeypatch, "%s, %s=%s" % (handle, switch[0], switch[1]), calls=calls)
    finally:
        monkeypatch.delenv(switch[0])
        fx[handle].tuning_reload()


def _oracle_clear(anchors):
    if not anchors:
        return []
    arr = (O.Sub * len(anchors))()
    for i, a in enumerate(anchors):
        arr[i].qbegin, arr[i].tbegin, arr[i].len, arr[i].trc, arr[i].qrc = a
    m = O.lib().lmo_clear_subs(arr, len(anchors), K)
    return [(arr[i].qbegin, arr[i].tbegin, arr[i].len, arr[i].trc, arr[i].qrc) for i in range(m)]


def _cmp_opt():
    opt = O.CmpOpt()
    opt.k, opt.min_prefix = 31, 11
    opt.c2.max_gap, opt.c2.min_score, opt.c2.min_align_len = 20, 35, 50
    opt.c2.min_identity, opt.c2.band_count, opt.c2.band_base, opt.c2.heuristic_pident = 70.0, 50, 100, 15.0
    return opt


def _oracle_chains(fx):
    """lmo_cmp_compare on the window text of every case, once"""
    if "oracle_chains" not in fx:
        L = O.lib()
        opt = _cmp_opt()
        cmps, out = {}, {}
        for i, c in enumerate(fx["cases"]):
            q = fx["queries"][c.q]
            if len(q) < K:
                out[i] = []
                continue
            if c.q not in cmps:
                cmps[c.q] = L.lmo_cmp_new(C.byref(opt))
                L.lmo_cmp_index(cmps[c.q], q, len(q))
            chains = C.POINTER(O.Chain2)()
            t = fx["res"][i].text
            nc = L.lmo_cmp_compare(cmps[c.q], c.qbegin, c.qend, t, len(t), len(q), C.byref(chains), None, None)
            out[i] = [(o.qbegin, o.qend, o.tbegin, o.tend, o.nanchors, o.matched_bases, o.aligned_bases_q, o.pident)
                      for o in (chains[j] for j in range(nc))]
            if nc:
                L.free(chains)
        for c in cmps.values():
            L.lmo_cmp_free(c)
        fx["oracle_chains"] = out
    return fx["oracle_chains"]


def _chain_tuples(chains):
    return [(g["qbegin"], g["qend"], g["tbegin"], g["tend"], g["nanchors"], g["matched_bases"], g["aligned_bases_q"], g["pident"])
            for g in chains]


@pytest.mark.parametrize("handle", ["dev", "host"])
def test_default_tuning_subset_same_clear_same_chains(fx, handle):
    exp = _oracle_chains(fx)
    idx, chains, anchors = _call(fx, fx[handle], "main")
    if handle == "dev":
        more = _call(fx, fx[handle], "many")
        idx, chains, anchors = idx + more[0], chains + more[1], anchors + more[2]
    emitted = raw = nchains = 0
    for i, ch, got in zip(idx, chains, anchors):
        r, c = fx["res"][i], fx["cases"][i]
        assert not collections.Counter(got) - collections.Counter(r.raw), c.name                  # a sub-multiset of raw
        assert _oracle_clear(got) == r.cleared, c.name                                            # nothing ClearSubstrPairs keeps is lost
        keys = [M.sort_key(a) for a in got]
        assert all(keys[j] <= keys[j + 1] for j in range(len(keys) - 1)), c.name
        assert _chain_tuples(ch) == exp[i], c.name                                                # integers exact, pident equal as a double
        emitted += len(got)
        raw += len(r.raw)
        nchains += len(ch)
    print("pa edges on the GPU (%s): %d anchors emitted with the rule on of %d raw, %d chains" % (handle, emitted, raw, nchains))
    assert 0 < emitted < raw and nchains >= 10


def test_ascii_windows_give_the_raw_list_and_the_same_chains(fx):
    """three ways on the same windows: packed genome, ASCII text, model (the ASCII path has no packed genome behind it: the
    nested-anchor rule does not apply, so it emits the raw list under the default tuning too)"""
    exp = _oracle_chains(fx)
    gi = fx["dev"]
    idx, chains_p, _ = _call(fx, gi, "main")
    idx2, chains_a, anchors_a = _call(fx, gi, "main", packed=False)
    assert idx == idx2
    _assert_raw(fx, idx, anchors_a, "ASCII windows")
    for i, a, b in zip(idx, chains_p, chains_a):
        assert a == b and _chain_tuples(a) == exp[i], fx["cases"][i].name
    # the plain entry point still returns these chains
    cases = [fx["cases"][i] for i in fx["calls"]["three_queries"]]
    used = sorted({c.q for c in cases})
    plain = gi.pseudoalign([fx["queries"][q] for q in used],
                           [(used.index(c.q), c.qbegin, c.qend, fx["res"][i].text) for i, c in zip(fx["calls"]["three_queries"], cases)])
    assert [_chain_tuples(p) for p in plain] == [exp[i] for i in fx["calls"]["three_queries"]]


def test_refused_arguments(fx):
    gi = fx["dev"]
    q = [fx["queries"][0]]
    glen = len(fx["fetched"][0])
    for region, text in (((0, 0, 599, len(fx["genomes"]), 0, 100, 0), "not a local genome"),
                         ((0, 0, 599, -1, 0, 100, 0), "not a local genome"),
                         ((0, 0, 599, 0, -1, 100, 0), "tbegin -1 < 0"),
                         ((0, 0, 599, 0, glen - 99, 100, 1), "past the genome's last base"),
                         ((0, 0, 601, 0, 0, 100, 0), "past the query"),
                         ((1, 0, 10, 0, 0, 100, 0), "query 1 of 1")):
        with pytest.raises(ValueError, match=text):
            gi.pseudoalign_regions(q, [region])
    # the edges of the legal range: the whole genome, qend == the query's length, an empty window, no region at all
    chains, anchors = gi.pseudoalign_regions(q, [(0, 0, 600, 0, 0, glen, 0), (0, 0, 600, 0, glen, 0, 1)])
    assert len(anchors[0]) > 0 and anchors[1] == [] and chains[1] == []
    assert gi.pseudoalign_regions(q, []) == ([], [])
    # the ASCII form takes both anchor outputs or neither
    la = _la()
    L = la.lib()
    qarr, keep = la.api._queries(q)
    one = (C.c_uint32 * 1)(0)
    sg, ro, rv, ao = C.c_void_p(), C.POINTER(C.c_int64)(), C.POINTER(la.api.Chain2)(), C.POINTER(C.c_int64)()
    st = L.lm_pseudoalign_batch_ex(gi.h, qarr, 1, qarr, one, one, (C.c_uint32 * 1)(599), 1, C.byref(sg), C.byref(ro), C.byref(rv),
                                   C.byref(ao), None)
    assert st == la.api.LM_ERR_ARG and not sg


def test_the_seam_runs_what_a_search_runs(fx, monkeypatch):
    """the windows a search opens, rebuilt from the seed chains (lm_seed_chain_batch) by the rule of the search (first / last
    anchor of every chain -+ ext_len, clipped at the genome's ends; lib-index-search.go:1967-2047), give through the seam as many
    windows as stats["chains"] counts and exactly the anchors stats["pa_anchors"] counts, with the rule off and on"""
    import random
    gi = fx["dev"]
    rng = random.Random(5)
    big = fx["fetched"][2]
    reads = []
    for at, n in ((100000, 2500), (180000, 1800), (60000, 3000)):
        s = bytearray(big[at:at + n])
        for j in range(40, n, 97):
            s[j] = rng.choice([b for b in b"ACGT" if b != s[j]])
        reads.append(bytes(s))
    reads[1] = M.revcomp_text(reads[1])
    ext = gi.opt.ext_len
    min_score = O.lib().lmo_seed_weight(float(gi.opt.min_single_prefix))
    assert gi.opt.top_n_genomes == 0 or gi.opt.top_n_genomes >= len(fx["genomes"])
    regions = []
    for p in gi.seed_chain(reads):
        if p["score"] < min_score:
            continue
        g = p["genome"] & 0x1ffff
        glen, qlen = len(fx["fetched"][g]), len(reads[p["query"]])
        sb = p["cleared"]  # (qbegin, tbegin, len, qrc, trc)
        tasks = []
        for ch in p["chains"]:
            first, last = sb[ch[0]], sb[ch[-1]]
            qb, tb = first[0], first[1]
            qe, te = last[0] + last[2] - 1, last[1] + last[2] - 1
            rc = (last[3] != last[4]) if len(ch) == 1 else tb > last[1]
            if rc:
                t0, t1 = max(last[1] - ext, 0), tb + last[2] - 1 + ext
            else:
                t0, t1 = max(tb - ext, 0), te + ext
            q0, q1 = qb - min(qb, ext), qe + min(qlen - qe - 1, ext)
            en = max(min(t1, glen - 1), t0)
            wlen = en - t0 + 1 if t0 < glen else 0
            tasks.append((tb, (p["query"], q0, q1, g, t0, wlen, int(rc))))
        tasks.sort(key=lambda t: t[0])  # (stable: chains by TBegin of their first anchor)
        regions += [t[1] for t in tasks]
    assert len(regions) >= 3 and {r[6] for r in regions} == {0, 1}
    for rule in ("0", "1"):
        monkeypatch.setenv("LM_PA_DROP_NESTED", rule)
        gi.tuning_reload()
        try:
            rows, st = gi.search(reads)
            _, anchors = gi.pseudoalign_regions(reads, regions)
        finally:
            monkeypatch.delenv("LM_PA_DROP_NESTED")
            gi.tuning_reload()
        assert len(rows) >= 3
        assert st["chains"] == len(regions)
        assert st["pa_anchors"] == sum(len(a) for a in anchors) > 0, rule
