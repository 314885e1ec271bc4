"""Indexes built on the GPU from caller-supplied masks (lm_index_builder_new_masks, Index.from_genomes(masks=...)): any k in
[10, 32], up to 32 masks on a p-base prefix.  Every mask list, info(), the rows and the genome bytes against the oracle's index
writer run on the same genomes with the same masks; the same index as the generated-mask path where both apply; save, open,
extend, join, subset and shards; the refusals.  Genomes: tests/genome_build_fixture.py; mask sets: tests/mask_sets.py."""
import filecmp
import os

import numpy as np
import pytest

import genome_build_fixture as F
import mask_sets as MS
import oracle as O

pytestmark = pytest.mark.gpu

ROW_FIELDS = ("batch_genome", "aligned_length", "qbegin", "qend", "tbegin", "tend", "bitscore", "gaps", "pident",
              "seq_idx", "nchunks", "chunk_idx", "genome_id", "seq_id")
INFO_FIELDS = ("seeds", "genomes", "genome_bases", "total_bases", "outlier_seeds")


def _la():
    import lexicmap_amd as la
    return la


def _bo(**kw):
    kw.setdefault("max_genome", F.MAX_GENOME)
    return _la().BuildOpt.default(**kw)


def _lists(ix, sample):
    out = {}
    for m in sample:
        k, v = ix.mask_seeds(m)
        out[m] = sorted(zip(k.tolist(), v.tolist()))
    return out


def _same_lists(a, b):
    assert sorted(a) == sorted(b)
    for m in a:
        assert a[m] == b[m], (m, len(a[m]), len(b[m]), [x for x in a[m] if x not in b[m]][:3], [x for x in b[m] if x not in a[m]][:3])


def _rows(ix, queries):
    rows, _ = ix.search(queries)
    return [[{f: r[f] for f in ROW_FIELDS} for r in rows if r["query"] == qi] for qi in range(len(queries))]


def _oracle_rows(d, queries):
    oi = O.Index(d)
    out = [[{f: r[f] for f in ROW_FIELDS} for r in oi.search(q)[0]] for q in queries]
    oi.close()
    return out


def _same_info(a, b, fields=INFO_FIELDS):
    for f in fields:
        assert a[f] == b[f], (f, a[f], b[f])


def _same_files(da, db):
    names, other = [], []
    for root, _, files in os.walk(da):
        names += [os.path.relpath(os.path.join(root, f), da) for f in files]
    for root, _, files in os.walk(db):
        other += [os.path.relpath(os.path.join(root, f), db) for f in files]
    assert sorted(names) == sorted(other) and "masks.bin" in names and len(names) >= 8
    _, mismatch, errors = filecmp.cmpfiles(da, db, names, shallow=False)
    assert not mismatch and not errors, (mismatch, errors)


def _oracle_index(tmp, name, gs, k, ms, **kw):
    d = str(tmp / (name + ".lmi"))
    O.build_index(d, gs, O.default_build_opt(k=k, chunks=4, max_genome=F.MAX_GENOME, masks=len(ms), **kw), masks=list(ms))
    return d


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    gs = F.genomes()
    return dict(gs=gs, queries=F.queries(gs), recs=F.records(gs), tmp=tmp_path_factory.mktemp("custom"))


def _against_the_oracles_writer(env, name, k, ms, sample=None, rows=True, options=None, fetch=True, nrows=None):
    """build with the caller's masks and hold the index to the oracle writer's of the same masks"""
    la = _la()
    assert len(ms) <= 2 * 4 ** MS.prefix_bases(len(ms))        # (the oracle's constructor needs that of the TOTAL)
    gi = la.Index.from_genomes(env["gs"], _bo(k=k), options=options, masks=ms)
    try:
        d = _oracle_index(env["tmp"], name, env["gs"], k, ms)
        oi = la.Index(d, options=options)
        try:
            assert gi.masks().tolist() == list(ms) == oi.masks().tolist()
            a, b = gi.info(), oi.info()
            _same_info(a, b)
            assert (a["k"], a["masks"], a["mask_prefix"], a["genomes"]) == (k, len(ms), MS.prefix_bases(len(ms)), 9)
            sample = range(len(ms)) if sample is None else sample
            got = _lists(gi, sample)
            _same_lists(got, _lists(oi, sample))
            assert {v >> 30 for kv in got.values() for _, v in kv} == set(range(9))
            if fetch:
                for l, (gid, contigs) in enumerate(env["recs"]):
                    exp = F.concatenation(contigs)
                    assert gi.fetch(l, 0, len(exp)) == exp, (l, gid)
            if rows:
                r, e = _rows(gi, env["queries"]), _oracle_rows(d, env["queries"])
                if nrows:       # (what the oracle's searcher was seen to give for this set when the case was chosen)
                    assert nrows[0] <= sum(len(x) for x in e) <= nrows[1], [len(x) for x in e]
                assert _rows(oi, env["queries"]) == r                  # built here or written by the oracle and opened: one index
                for qi, (x, y) in enumerate(zip(r, e)):
                    assert x == y, (qi, x, y)
                assert sum(len(x) for x in e) > 0
            return got, a
        finally:
            oi.close()
    finally:
        gi.close()


def _desert_seeds(lists):
    """(mask, record) pairs holding more than one forward k-mer: desert seeds"""
    n = 0
    for kv in lists.values():
        per = {}
        for k, v in kv:
            if not v & 1:
                per.setdefault(v >> 30, set()).add(k)
        n += sum(1 for s in per.values() if len(s) > 1)
    return n


# ---- 1. parity with the oracle's writer
@pytest.mark.parametrize("k,n", [(31, 500), (21, 24), (27, 2048), (32, 500)])
def test_skewed_sets_give_the_oracle_writers_index(env, k, n):
    """few masks leave thousands of seed deserts: the desert kernel runs with many masks on a prefix, the capture with the
    prefix table (three or more masks on the fullest prefix: asserted, so that a generator change cannot turn these into
    once-or-twice sets)"""
    ms = MS.skewed(k, n)
    assert max(MS.per_prefix(k, ms)) >= 3 and min(MS.per_prefix(k, ms)) >= 1
    got, info = _against_the_oracles_writer(env, "skew_%d_%d" % (k, n), k, ms, rows=False)
    assert _desert_seeds(got) > 100


@pytest.mark.parametrize("k,n", [(31, 500), (21, 24), (27, 2048), (32, 500)])
def test_skewed_sets_give_the_oracles_rows(env, k, n):
    """the rows of the fixture's six queries against the oracle's searcher on the oracle writer's index of the same masks
    (query 5 runs across 2000 A: it is the one that showed that the pseudo-alignment must compare 31-mers at every index k)"""
    ms = MS.skewed(k, n)
    _against_the_oracles_writer(env, "skewr_%d_%d" % (k, n), k, ms, sample=[0], fetch=False, nrows=(7, 8))


# ---- 2. tall and tiny
def test_32_masks_on_one_prefix_3_on_another_one_on_each_of_the_rest(env):
    ms = MS.tall_and_tiny(31)
    c = MS.per_prefix(31, ms)
    assert len(ms) == 97 and sorted(c) == [1] * 62 + [3, 32]
    got, _ = _against_the_oracles_writer(env, "tall", 31, ms)
    assert _desert_seeds(got) > 100


# ---- 3. beyond LDS, and the default count
@pytest.mark.parametrize("n", [24_000, 20_000])
def test_prefix_table_with_the_minima_in_a_global_table_and_in_lds(env, n):
    """24 000 masks: the minima do not fit a CU's LDS (global minima, prefix table in LDS); 20 000: the minima fill the LDS
    (prefix table in global memory).  Sampled lists, info() and rows as test_gpu_build_genomes.py does for 24 000 generated masks."""
    ms = MS.skewed(31, n)
    assert max(MS.per_prefix(31, ms)) >= 3 and (len(ms) * 8 > 160 * 1024) == (n == 24_000)
    sample = list(range(0, len(ms), 7)) + [len(ms) - 1]
    got, _ = _against_the_oracles_writer(env, "big_%d" % n, 31, ms, sample=sample, fetch=False, nrows=(7, 8) if n == 20_000 else None)
    for key in (3, 8):   # G4 and G8 under (nearly) every mask: the missing-prefix rule
        assert sum(1 for kv in got.values() if any((v >> 30) == key and not v & 1 for _, v in kv)) > 0.9 * len(got)


# ---- 4. the same index as before, where both paths apply
@pytest.mark.parametrize("n", [1024, 20_000])
def test_a_generated_set_given_back_as_the_callers_gives_the_same_files(env, n):
    """every prefix once or twice: the unchanged instantiation runs, and the saved indexes are equal byte for byte"""
    la = _la()
    gen = la.Index.from_genomes(env["gs"], _bo(masks=n))
    try:
        ms = gen.masks()
        assert ms.dtype == np.uint64 and len(ms) == n and max(MS.per_prefix(31, ms.tolist())) <= 2
        giv = la.Index.from_genomes(env["gs"], _bo(masks=4), masks=ms)      # (bo.masks is ignored: nmasks rules)
        try:
            _same_info(gen.info(), giv.info(), INFO_FIELDS + ("k", "masks", "mask_prefix", "key_bits", "seed_bytes"))
            sample = range(n) if n <= 1024 else list(range(0, n, 7)) + [n - 1]
            _same_lists(_lists(gen, sample), _lists(giv, sample))
            da, db = str(env["tmp"] / ("gen%d.lmi" % n)), str(env["tmp"] / ("giv%d.lmi" % n))
            gen.save(da, chunks=4)
            giv.save(db, chunks=4)
            _same_files(da, db)
        finally:
            giv.close()
    finally:
        gen.close()


# ---- 5. save, open, extend, join, subset, shard
@pytest.fixture(scope="module", params=[(21, 24), (31, 500)], ids=["k21_24", "k31_500"])
def built(request, env):
    la = _la()
    k, n = request.param
    ms = MS.skewed(k, n)
    gs = env["gs"]
    full = la.Index.from_genomes(gs, _bo(k=k), masks=ms)
    A = la.Index.from_genomes(gs[:4], _bo(k=k), masks=ms)
    B = la.Index.from_genomes(gs[4:], _bo(k=k), masks=ms)
    sample = range(len(ms))
    out = dict(k=k, ms=ms, full=full, A=A, B=B, sample=sample, lists=_lists(full, sample), rows=_rows(full, env["queries"]),
               dir=str(env["tmp"] / ("full_%d.lmi" % k)))
    full.save(out["dir"], chunks=3)
    yield out
    for ix in (full, A, B):
        ix.close()


def _same_index(got, built, env, tag):
    _same_info(got.info(), built["full"].info())
    _same_lists(_lists(got, built["sample"]), built["lists"])
    assert _rows(got, env["queries"]) == built["rows"]
    d = str(env["tmp"] / ("%s_%d.lmi" % (tag, built["k"])))
    got.save(d, chunks=3)
    _same_files(d, built["dir"])


def test_save_and_open(built, env):
    la = _la()
    li = la.Index(built["dir"])
    try:
        assert li.masks().tolist() == built["ms"] and li.info()["k"] == built["k"]
        _same_info(li.info(), built["full"].info())
        _same_lists(_lists(li, built["sample"]), built["lists"])
        assert _rows(li, env["queries"]) == built["rows"]
    finally:
        li.close()
    info = open(os.path.join(built["dir"], "info.toml")).read()
    assert "masks = %d\n" % len(built["ms"]) in info and "rand-seed = 1\n" in info
    assert sum(len(r) for r in built["rows"]) >= 6
    for qi, (x, y) in enumerate(zip(_oracle_rows(built["dir"], env["queries"]), built["rows"])):
        assert x == y, (qi, x, y)


def test_join_equals_one_build_of_all(built, env):
    j = built["A"].join(built["B"])
    try:
        _same_index(j, built, env, "join")
    finally:
        j.close()


def test_extend_equals_one_build_of_all(built, env):
    e = built["A"].extend(env["gs"][4:], _bo(k=built["k"], masks=len(built["ms"])))
    try:
        _same_index(e, built, env, "ext")
    finally:
        e.close()


def test_subset_equals_a_build_of_those_genomes(built, env):
    la = _la()
    s = built["full"].subset([0, 1, 2, 3])          # the records of G1 .. G4: what A was built from
    try:
        _same_info(s.info(), built["A"].info())
        _same_lists(_lists(s, built["sample"]), _lists(built["A"], built["sample"]))
        assert _rows(s, env["queries"]) == _rows(built["A"], env["queries"])
    finally:
        s.close()
    with pytest.raises(ValueError) as ei:            # the mutual checks are unchanged
        other = la.Index.from_genomes(env["gs"][3:4], _bo(k=built["k"]), masks=MS.skewed(built["k"], len(built["ms"]), seed=2))
        try:
            la.IndexBuilder.like(built["full"]).add_index(other)
        finally:
            other.close()
    assert "mask values differ" in str(ei.value)


def test_an_opened_index_is_a_base_a_model_and_a_source(built, env):
    """an index opened from disk with k = 21 (or with many masks on a prefix) can be extended, taken as a model and joined"""
    la = _la()
    d = _oracle_index(env["tmp"], "half_%d" % built["k"], env["gs"][:4], built["k"], built["ms"])
    opened = la.Index(d)
    try:
        _same_lists(_lists(opened, built["sample"]), _lists(built["A"], built["sample"]))
        b = la.IndexBuilder.like(opened)
        try:
            same = b.add_index(opened).finish()
        finally:
            b.close()
        try:
            _same_info(same.info(), built["A"].info())
            _same_lists(_lists(same, built["sample"]), _lists(built["A"], built["sample"]))
        finally:
            same.close()
        e = opened.extend(env["gs"][4:], _bo(k=built["k"], masks=len(built["ms"])))      # (max_genome splits G6 as in the full build)
        try:
            _same_info(e.info(), built["full"].info())
            _same_lists(_lists(e, built["sample"]), built["lists"])
            assert _rows(e, env["queries"]) == built["rows"]
        finally:
            e.close()
    finally:
        opened.close()


def test_two_shards_hold_the_unsharded_lists_and_merge_to_the_unsharded_rows(built, env):
    la = _la()
    from lexicmap_amd import merge
    tb = built["full"].info()["total_bases"]
    shards = [la.Index.from_genomes(env["gs"], _bo(k=built["k"]), masks=built["ms"],
                                    options=la.api.default_options(shard_rank=r, shard_count=2, total_bases_override=tb)) for r in range(2)]
    try:
        parts = [_lists(s, built["sample"]) for s in shards]
        assert {m: sorted(parts[0][m] + parts[1][m]) for m in built["sample"]} == built["lists"]
        assert [{v >> 30 for kv in p.values() for _, v in kv} for p in parts] == [{0, 2, 4, 8}, {1, 3, 5, 6, 7}]
        per_rank = []
        for s in shards:
            qb = s.upload(env["queries"])
            arr, _ = s.search_resident_np(qb)
            per_rank.append(arr.copy())
            s.free_batch(qb)
        merged, names = merge.merge_sharded_c(per_rank, shards[0])
        rows_w, _ = built["full"].search(env["queries"])
        assert len(merged) == len(rows_w) >= 6
        for i, w in enumerate(rows_w):
            for f in ("query", "hits", "batch_genome", "aligned_length", "qbegin", "qend", "tbegin", "tend", "bitscore", "gaps", "pident", "evalue"):
                assert merged[f][i] == w[f], (i, f)
            assert names[i] == (w["genome_id"], w["seq_id"]), i
    finally:
        for s in shards:
            s.close()


def test_seed_positions_are_those_read_off_the_lists(env):
    la = _la()
    ms = MS.skewed(31, 500)
    gi = la.Index.from_genomes(env["gs"], _bo(), masks=ms)
    try:
        v = np.concatenate([gi.mask_seeds(m)[1] for m in range(len(ms))])
        got = gi.seed_positions()
    finally:
        gi.close()
    v = v[(v & np.uint64(1)) == 0]
    assert len(got) == 9
    for key in range(9):
        exp = np.sort(((v[(v >> np.uint64(30)) == np.uint64(key)] >> np.uint64(1)) & np.uint64((1 << 29) - 1)).astype(np.uint32))
        assert len(exp) > 0 and np.array_equal(got[key], exp), key


# ---- 6. more masks than 2 * 4^p
def _kmers(seq, k):
    """(forward, reverse-complement) k-mer codes of every position, as Python ints"""
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    full = (1 << (2 * k)) - 1
    f = r = 0
    fw, rc = [], []
    for i, c in enumerate(seq):
        b = code[c]
        f = ((f << 2) | b) & full
        r = (r >> 2) | ((3 - b) << (2 * (k - 1)))
        if i >= k - 1:
            fw.append(f)
            rc.append(r)
    return fw, rc


def test_40000_masks_rows_by_the_oracles_searcher_and_forward_seeds_of_g4_by_brute_force(env):
    """p = 7 and up to 32 masks on a prefix: the oracle's WRITER cannot be made for this count (its constructor needs masks <=
    2 * 4^p), so the lists are not held to it.  Held instead: the rows, to the oracle's searcher on the saved index; and every
    forward seed of G4 (6 kb, ACGT only) of a build without desert filling, to a brute-force minimum of mask ^ k-mer over the
    k-mers of both strands that share the mask's prefix, or over all of them when none does.  Only this direction: a mask
    without a seed for G4 is allowed (low-complexity captures are dropped)."""
    la = _la()
    k = 31
    ms = MS.skewed(k, 40_000)
    c = MS.per_prefix(k, ms)
    assert len(ms) > 2 * 4 ** 7 and MS.prefix_bases(len(ms)) == 7 and 3 <= max(c) <= 32 and min(c) >= 1
    gi = la.Index.from_genomes(env["gs"], _bo(), masks=ms)
    try:
        d = str(env["tmp"] / "m40000.lmi")
        gi.save(d, chunks=4)
        rows = _rows(gi, env["queries"])
        assert rows == _oracle_rows(d, env["queries"]) and all(len(r) > 0 for r in rows)
    finally:
        gi.close()
    g4 = dict(env["gs"])["G4"][0][1]
    fw, rc = _kmers(g4, k)
    allk = np.array(fw + rc, dtype=np.uint64)
    by_prefix = {}
    for x in fw + rc:
        by_prefix.setdefault(x >> (2 * (k - 7)), []).append(x)
    by_prefix = {p: np.array(v, dtype=np.uint64) for p, v in by_prefix.items()}
    gi = la.Index.from_genomes(env["gs"], _bo(max_desert=2 ** 27), masks=ms)
    try:
        checked = missing_rule = 0
        for m in list(range(0, len(ms), 7)) + [len(ms) - 1]:
            kk, vv = gi.mask_seeds(m)
            cand = by_prefix.get(ms[m] >> (2 * (k - 7)))
            best = None
            for x, v in zip(kk.tolist(), vv.tolist()):
                if (v >> 30) != 3 or v & 1:
                    continue
                pos, strand = (v >> 2) & ((1 << 28) - 1), (v >> 1) & 1
                assert (rc if strand else fw)[pos] == x, (m, pos, strand)
                if best is None:
                    best = int((np.uint64(ms[m]) ^ (cand if cand is not None else allk)).min())
                    missing_rule += cand is None
                assert ms[m] ^ x == best, (m, pos, strand)
                checked += 1
        assert checked > 5000 and missing_rule > 2000      # 2 x 5970 k-mers meet 16384 prefixes: most masks take the rule
    finally:
        gi.close()


# ---- 7. k = 12
def test_k_12_lists_equal_the_oracle_writers(env):
    la = _la()
    ms = MS.tall_and_tiny(12)
    opt = la.api.default_options(min_prefix=10, min_single_prefix=12)      # p + anchor_prefix = 9 <= min_prefix <= k
    _against_the_oracles_writer(env, "k12", 12, ms, rows=False, options=opt)


# ---- 8. refusals
def test_refusals_name_the_offender_and_a_good_set_builds_afterwards(env):
    la = _la()
    good = MS.skewed(31, 500)
    tall33 = MS.tall_and_tiny(31, tall=33)
    cases = [
        (31, good[:100] + [good[100], good[99]] + good[102:], "mask 101 "),            # not ascending
        (31, good[:7] + [good[6]] + good[8:], "mask 7 equals mask 6"),                 # a duplicate
        (21, MS.skewed(21, 24)[:-1] + [4 ** 21], "mask %d " % (len(MS.skewed(21, 24)) - 1)),    # >= 4^k
        (31, [m for m in good if m >> 54 != 200], "prefix 200 "),                      # an empty prefix
        (31, tall33, "prefix 5 has 33 masks"),
        (9, [0, 1 << 16, 2 << 16, 3 << 16], "k = 9"),
        (33, [0, 1 << 62, 2 << 62, 3 << 62], "k = 33"),
        (31, [0, 1 << 60, 2 << 60], "3 masks"),
        (31, np.arange(65536, dtype=np.uint64) << np.uint64(40), "65536 masks"),
    ]
    for k, ms, word in cases:
        with pytest.raises(ValueError) as ei:
            la.IndexBuilder(_bo(k=k), masks=ms)
        assert ei.value.status == 7 and word in str(ei.value), (word, str(ei.value))
        assert word in la.lib().lm_last_error(None).decode()
    gi = la.Index.from_genomes(env["gs"][3:4], _bo(), masks=good)
    try:
        assert gi.info()["masks"] == len(good) and gi.info()["seeds"] > 0
    finally:
        gi.close()
