"""Seed positions and seed distances of a resident index (lm_index_seed_positions / lm_index_seed_distances,
Index.seed_positions / seed_distances).  Yardstick of the positions: the oracle-checked Index.mask_seeds - for every mask
the values with bit 0 clear, record value >> 30, loc (value >> 1) & (2^29 - 1), sorted per record in numpy.  Yardstick of
the distances: the rule of DESIGN.md section 11 restated in numpy from the fixture's contig lengths and the contig interval.
Fixture set: tests/genome_build_fixture.py (9 records; G2 = record 1 has four contigs, one shorter than k)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import genome_build_fixture as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROW_FIELDS = ("record", "contig", "pos", "pos_in_contig", "strand", "dist")
REC_FIELDS = ("key", "seeds", "max_dist", "max_dist_pos", "contigs", "contigs_without_seeds")
HSP_FIELDS = ("query", "batch_genome", "aligned_length", "qbegin", "qend", "tbegin", "tend", "bitscore", "gaps", "pident", "hsp", "cls")


def _la():
    import lexicmap_amd as la
    return la


def _bo(**kw):
    return _la().BuildOpt.default(max_genome=F.MAX_GENOME, **kw)


def yardstick(ix):
    """{record key: sorted uint32 locs} from one mask_seeds call per mask"""
    vals = [ix.mask_seeds(m)[1] for m in range(ix.info()["masks"])]
    v = np.concatenate(vals)
    v = v[(v & np.uint64(1)) == 0]
    rec = v >> np.uint64(30)
    loc = ((v >> np.uint64(1)) & np.uint64((1 << 29) - 1)).astype(np.uint32)
    order = np.lexsort((loc, rec))
    rec, loc = rec[order], loc[order]
    keys, first = np.unique(rec, return_index=True)
    return {int(k): a for k, a in zip(keys, np.split(loc, first[1:]))}


def _same(got, want, what=""):
    assert got.dtype == np.uint32 and len(got) == len(want), (what, len(got), len(want))
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:5])


def _same_as_yardstick(lists, yard, keys):
    assert len(lists) == len(keys)
    for got, k in zip(lists, keys):
        _same(got, yard[k], k)


def _keys(ix):
    return [int(k) for k in ix.seed_distances()["records"]["key"]]


def _rows(ix, queries):
    rows, _ = ix.search(queries)
    return [{f: r[f] for f in HSP_FIELDS} for r in rows]


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    la = _la()
    gs = F.genomes()
    full = la.Index.from_genomes(gs, _bo(masks=1024))
    out = dict(gs=gs, recs=F.records(gs), full=full, yard=yardstick(full), tmp=tmp_path_factory.mktemp("seedpos"))
    yield out
    full.close()


# ---- 1. the fixture set with 1024 masks (thousands of desert seeds), every record and a selection; 4. the outlier path
def test_positions_of_the_fixture_build(fx):
    full, yard = fx["full"], fx["yard"]
    info = full.info()
    assert info["genomes"] == 9 and info["outlier_seeds"] > 0          # (G4 and G8 lack most mask prefixes: the flat lists run)
    assert sorted(yard) == list(range(9))
    lists = full.seed_positions()
    _same_as_yardstick(lists, yard, list(range(9)))
    assert 2 * sum(len(a) for a in lists) == info["seeds"]           # every forward seed has its reversed twin
    assert any(len(np.unique(a)) < len(a) for a in lists)             # a position captured by two masks stays twice
    _same_as_yardstick(full.seed_positions([7, 2, 5]), yard, [7, 2, 5])
    _same_as_yardstick(full.seed_positions([8]), yard, [8])           # the 200-base genome: nearly every wavefront keeps nothing


# ---- 2. pieces far smaller than a record's seeds, cut inside lists and tiles (the switch is read in a fresh process)
CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import genome_build_fixture as F
import lexicmap_amd as la
ix = la.Index.from_genomes(F.genomes(), la.BuildOpt.default(max_genome=F.MAX_GENOME, masks=1024))
a, b = ix.seed_positions(), ix.seed_positions([7, 2, 5])
d = ix.seed_distances([7, 2, 5], min_dist=200, bins=16, bin_width=10)
np.savez(sys.argv[3], *(a + b), rows=d["rows"], hist=d["hist"], records=d["records"])
ix.close()
"""


def test_positions_in_small_pieces(fx):
    full, yard = fx["full"], fx["yard"]
    longest = max(int(np.count_nonzero((full.mask_seeds(m)[1] & np.uint64(1)) == 0)) for m in range(0, 1024, 16))
    # A third of a forward list that exists: that list spans at least three pieces, so at least two piece ends fall INSIDE it,
    # and a piece is shorter than a tile of 256 seeds, so those ends - and the end of nearly every other piece - fall inside a
    # tile: the kernel's tile brackets begin and end in the middle of a list.
    piece = max(4, longest // 3)
    assert 3 * piece <= longest and piece < 256
    # every record's seeds span several pieces (record 8, the 200-base genome, has fewer seeds than that and is left out here:
    # its list is still compared below)
    assert min(len(a) for k, a in yard.items() if k != 8) > 8 * piece
    out = str(fx["tmp"] / "pieces.npz")
    env = dict(os.environ, LM_SEEDPOS_PIECE_SEEDS=str(piece), LM_DEBUG="1")
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, HERE, out], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "pieces of %d," % piece in r.stderr
    z = np.load(out)
    got = [z["arr_%d" % i] for i in range(12)]
    _same_as_yardstick(got[:9], yard, list(range(9)))
    _same_as_yardstick(got[9:], yard, [7, 2, 5])
    want = full.seed_distances([7, 2, 5], min_dist=200, bins=16, bin_width=10)
    for f in ("rows", "hist", "records"):
        assert np.array_equal(z[f], want[f]), f


# ---- 3. 20 000 masks: long forward lists, several partitions per tile
def test_positions_with_20000_masks(fx):
    ix = _la().Index.from_genomes(fx["gs"], _bo(masks=20000))
    try:
        yard = yardstick(ix)
        _same_as_yardstick(ix.seed_positions(), yard, list(range(9)))
    finally:
        ix.close()


# ---- 5. distances
def np_distances(contig_lens, lists, min_dist, bins, width, interval=F.CONTIG_INTERVAL):
    """the rule restated: contig_lens[slot] = lengths of the record's contigs, lists[slot] = its sorted locs"""
    rows, recs, hist = [], [], np.zeros(bins, np.uint64)
    for slot, (lens, loc) in enumerate(zip(contig_lens, lists)):
        lens = np.asarray(lens, np.int64)
        starts = np.concatenate([[0], np.cumsum(lens + interval)[:-1]])
        p = (loc >> 1).astype(np.int64)
        c = np.searchsorted(starts, p, side="right") - 1
        first = np.ones(len(p), bool)
        first[1:] = c[1:] != c[:-1]
        dist = np.where(first, p - starts[c], p - np.concatenate([[0], p[:-1]]))
        keep = dist >= min_dist
        rows.append(np.stack([np.full(keep.sum(), slot), c[keep], p[keep], (p - starts[c])[keep], (loc & 1)[keep], dist[keep]], axis=1))
        if bins:
            hist += np.bincount(np.minimum(dist[keep] // width, bins - 1), minlength=bins).astype(np.uint64)
        top = int(np.argmax(dist)) if len(p) else 0
        recs.append((len(p), int(dist[top]) if len(p) else 0, int(p[top]) if len(p) else 0, len(lens), len(lens) - len(np.unique(c))))
    return np.concatenate(rows), recs, hist


def _check_distances(got, keys, contig_lens, lists, min_dist, bins, width):
    rows, recs, hist = np_distances(contig_lens, lists, min_dist, bins, width)
    g = np.stack([got["rows"][f].astype(np.int64) for f in ROW_FIELDS], axis=1) if len(got["rows"]) else np.zeros((0, 6), np.int64)
    assert g.shape == rows.shape and np.array_equal(g, rows), (g.shape, rows.shape)
    assert [int(k) for k in got["records"]["key"]] == list(keys)
    assert [tuple(int(r[f]) for f in REC_FIELDS[1:]) for r in got["records"]] == recs
    assert np.array_equal(got["hist"], hist) and len(got["hist"]) == bins
    return g


@pytest.mark.parametrize("keys", [None, [7, 1, 4, 2, 8]])   # (G3 = 2 and G5 = 4 hold the distances of 200 and more)
def test_distances_equal_the_restated_rule(fx, keys):
    full = fx["full"]
    sel = list(range(9)) if keys is None else keys
    lens = [[len(s) for _, s in fx["recs"][k][1]] for k in sel]
    lists = [fx["yard"][k] for k in sel]
    nseeds = sum(len(a) for a in lists)
    all_rows = _check_distances(full.seed_distances(keys, min_dist=0, bins=16, bin_width=10), sel, lens, lists, 0, 16, 10)
    assert len(all_rows) == nseeds
    d200 = full.seed_distances(keys, min_dist=200, bins=16, bin_width=10)
    far = _check_distances(d200, sel, lens, lists, 200, 16, 10)
    assert 0 < len(far) < nseeds and int(d200["hist"][:15].sum()) == 0 and int(d200["hist"][15]) == len(far)
    assert {tuple(r) for r in far} < {tuple(r) for r in all_rows}      # a strict subset of the rows of min_dist = 0
    assert len(_check_distances(full.seed_distances(keys), sel, lens, lists, 0, 0, 0)) == nseeds   # no histogram asked for
    # the multi-contig record G2 (key 1): pos_in_contig restarts, the 25-base contig holds no seed, and the first row of
    # every seeded contig has dist = pos - s_c
    slot = sel.index(1)
    r = all_rows[all_rows[:, 0] == slot]
    assert sorted(set(r[:, 1])) == [0, 2, 3]
    starts = [0, 61_000, 62_025, 64_225]
    for c in (0, 2, 3):
        rc = r[r[:, 1] == c]
        assert rc[0, 5] == rc[0, 2] - starts[c] == rc[0, 3] and np.all(rc[:, 3] == rc[:, 2] - starts[c])
        assert np.all(rc[1:, 5] == np.diff(rc[:, 2]))
    for c in (2, 3):
        assert r[r[:, 1] == c][0, 3] < r[r[:, 1] == c - (2 if c == 2 else 1)][-1, 3]   # restarted below the contig before
    rec = full.seed_distances(keys)["records"][slot]
    assert rec["contigs"] == 4 and rec["contigs_without_seeds"] == 1


# ---- 6. the same index by other routes
def test_other_routes_give_the_same_lists(fx):
    la = _la()
    gs, full, yard, tmp = fx["gs"], fx["full"], fx["yard"], fx["tmp"]
    A, B = gs[:5], gs[5:]
    a, b = la.Index.from_genomes(A, _bo(masks=1024)), la.Index.from_genomes(B, _bo(masks=1024))
    opened = [a, b]
    try:
        _same_as_yardstick(a.seed_positions(), yard, [0, 1, 2, 3, 4])
        _same_as_yardstick(b.seed_positions(), yard, [5, 6, 7, 8])     # b numbers them 0..3
        assert _keys(b) == [0, 1, 2, 3]
        for ix in (a.extend(B, _bo(masks=1024)), a.join(b)):           # (extend splits G6 at the fixture's max_genome)
            opened.append(ix)
            assert _keys(ix) == list(range(9))
            _same_as_yardstick(ix.seed_positions(), yard, list(range(9)))
            _same_as_yardstick(ix.seed_positions([6, 0]), yard, [6, 0])
        d = dict(gs)
        kept = la.Index.from_genomes([(n, d[n]) for n in ("G1", "G3", "G6", "G8")], _bo(masks=1024))
        sub = full.subset([8, 2, 6, 0, 5])
        opened += [kept, sub]
        assert _keys(sub) == _keys(kept) == [0, 1, 2, 3, 4]
        want = kept.seed_positions()
        _same_as_yardstick(want, yard, [0, 2, 5, 6, 8])                # the records' old keys in the full build
        for g, w in zip(sub.seed_positions(), want):
            _same(g, w)
        _same(sub.seed_positions([3])[0], yard[6])
        # saved and opened again, genomes on the device and in pinned host memory
        path = str(tmp / "full2.lmi")
        full.save(path, chunks=3)
        o1 = la.Index(path)
        opened.append(o1)
        o2 = la.Index(path, residency=la.api.Residency(la.api.GENOMES_HOST))
        opened.append(o2)
        assert o2.residency()["genomes_host"] == 9 and o2.residency()["genomes_device"] == 0
        for ix in (o1, o2):
            assert _keys(ix) == list(range(9))
            _same_as_yardstick(ix.seed_positions(), yard, list(range(9)))
        assert np.array_equal(o2.seed_distances(min_dist=100)["rows"], full.seed_distances(min_dist=100)["rows"])
    finally:
        for ix in opened:
            ix.close()


# ---- 7. shards
def test_shards_answer_for_their_own_records(fx):
    la = _la()
    yard = fx["yard"]
    seen = []
    for rank in (0, 1):
        sh = la.Index.from_genomes(fx["gs"], _bo(masks=1024), options=la.api.default_options(shard_rank=rank, shard_count=2))
        try:
            keys = _keys(sh)
            assert keys == sorted(keys) and len(keys) == sh.info()["genomes"] > 0
            _same_as_yardstick(sh.seed_positions(), yard, keys)
            _same_as_yardstick(sh.seed_positions(keys[::-1][:2]), yard, keys[::-1][:2])
            foreign = next(k for k in range(9) if k not in keys)
            with pytest.raises(ValueError) as ei:
                sh.seed_positions([keys[0], foreign])
            assert "another shard" in str(ei.value) and "shard %d of 2" % rank in str(ei.value)
            with pytest.raises(ValueError):
                sh.seed_distances([foreign])
            _same_as_yardstick(sh.seed_positions([keys[0]]), yard, [keys[0]])   # the handle still answers
            seen += keys
        finally:
            sh.close()
    assert sorted(seen) == list(range(9))                               # the union is the unsharded set


# ---- 8. refusals leave the handle usable
def test_refusals(fx):
    full = fx["full"]
    q = F.queries(fx["gs"])[:1]
    before = _rows(full, q)
    assert len(before) > 0
    for call, word in ((lambda: full.seed_positions([0, 99]), "no record of this index"),
                       (lambda: full.seed_positions([3, 1, 3]), "twice"),
                       (lambda: full.seed_distances([3, 1, 3]), "twice"),
                       (lambda: full.seed_distances(bins=4, bin_width=0), "hist_width")):
        with pytest.raises(ValueError) as ei:
            call()
        assert word in str(ei.value), str(ei.value)
        assert _rows(full, q) == before
    _same_as_yardstick(full.seed_positions([4]), fx["yard"], [4])
    # an empty list of keys selects nothing (None selects everything)
    assert full.seed_positions([]) == []
    d = full.seed_distances([], min_dist=0, bins=4, bin_width=10)
    assert len(d["records"]) == 0 and len(d["rows"]) == 0 and d["hist"].tolist() == [0, 0, 0, 0]
