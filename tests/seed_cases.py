"""Seeded fixtures of the seed-lookup / seed-chaining edge tests (test_seed_edges_cpu.py, test_gpu_seed_edges.py): indexes
made of one ordinary genome and many tiny ones, and the named queries searched in them.  Test infrastructure only.

An index of viruses, plasmids or genes holds tiny genomes only.  A tiny genome lacks most of the masks' prefixes, so what it
leaves under a mask is a k-mer of another prefix: an OUTLIER of the mask's list (the packed image keeps those flat, beside the
partitions), and a second run of some anchor bases in the reference's list, which hides the first one from the reference's
anchor index (seed_model.py: the start rule).

  V20k  one random 120-kb genome + 150 random genomes of 200-3000 bases, the default 20 000 masks
  V2k   the same genomes, 2000 masks (other mask prefix, key and table widths)
  C2k   one 120-kb genome + 80 copies of one 1.5-kb genome at about 1 % substitutions, 2000 masks: lookups that return 65
        values and more, some of them from outlier lists (a 3-kb genome holds nearly every 5-base prefix: its copies gave
        4138 such lookups, none of them an outlier lookup; at 1.5 kb the defaults give 8)
  K21   one 120-kb genome + 20 tiny ones, 2000 masks, k = 21

Every sequence comes from Python's Mersenne Twister (random.Random(seed).getrandbits), whose stream is fixed across versions:
the windows in CHAIN_WINDOWS were chosen against exactly these genomes (tests/seed_cases.py scan(), run once on the CPU with
the oracle) and the CPU test asserts that they still give the pair sizes they were chosen for.
"""
import os
import random

import numpy as np

import oracle as O

COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def revcomp(s):
    return s.translate(COMP)[::-1]


def random_seq(rng, n):
    """n random bases from a random.Random"""
    raw = np.frombuffer(rng.getrandbits(8 * n).to_bytes(n, "little"), dtype=np.uint8)
    return _ACGT[raw & 3].tobytes()


def substitute(rng, s, rate):
    b = bytearray(s)
    for i in range(len(b)):
        if rng.random() < rate:
            b[i] = b"ACGT"[(b"ACGT".index(b[i]) + rng.randint(1, 3)) & 3]
    return bytes(b)


def tiny_genomes(seed, ntiny, big_len=120_000, len_range=(200, 3000)):
    """[("B0", [("b0", 120 kb)]), ("T0", [("t0", 200-3000 bases)]), ...]"""
    rng = random.Random(seed)
    genomes = [("B0", [("b0", random_seq(rng, big_len))])]
    for i in range(ntiny):
        genomes.append(("T%d" % i, [("t%d" % i, random_seq(rng, rng.randint(*len_range)))]))
    return genomes


def copy_genomes(seed, ncopies=80, copy_len=1500, rate=0.01):
    rng = random.Random(seed)
    genomes = [("B0", [("b0", random_seq(rng, 120_000))])]
    base = random_seq(rng, copy_len)
    for i in range(ncopies):
        genomes.append(("C%d" % i, [("c%d" % i, substitute(rng, base, rate))]))
    return genomes


# ---- the oracle's side, read through numpy views (a pair here holds up to 40 000 anchors)
ANCHOR_DTYPE = np.dtype([("genome", "<u8"), ("qbegin", "<i4"), ("tbegin", "<i4"), ("len", "u1"), ("trc", "u1"), ("qrc", "u1"),
                         ("pad", "u1"), ("pad2", "<u4")])
SUB_DTYPE = np.dtype([("qbegin", "<i4"), ("tbegin", "<i4"), ("len", "u1"), ("trc", "u1"), ("qrc", "u1"), ("pad", "u1")])
FIELDS = ("qbegin", "tbegin", "len", "qrc", "trc")


def stage_mask(oi, seq):
    """captured k-mers [M], location offsets [M + 1] and locations (position << 1 | strand) of one query (lmo_stage_mask)"""
    import ctypes as C
    L, M = O.lib(), oi.nmasks
    ok = (C.c_uint64 * M)()
    ooff, olocs = C.POINTER(C.c_int)(), C.POINTER(C.c_int)()
    assert L.lmo_stage_mask(oi.h, seq, len(seq), ok, C.byref(ooff), C.byref(olocs)) == 0
    off = np.ctypeslib.as_array(ooff, shape=(M + 1,)).astype(np.int64)
    locs = np.ctypeslib.as_array(olocs, shape=(max(int(off[M]), 1),)).astype(np.int64)[:int(off[M])]
    L.free(ooff)
    L.free(olocs)
    return np.frombuffer(ok, dtype=np.uint64).copy(), off, locs


def oracle_anchors(oi, seq, k=31):
    """the oracle's seed anchors of one query (lmo_stage_anchors): sorted by genome, ClearSubstrPairs order within one"""
    import ctypes as C
    assert C.sizeof(O.Anchor) == ANCHOR_DTYPE.itemsize
    if len(seq) < k:
        return np.zeros(0, dtype=ANCHOR_DTYPE)
    L, M = O.lib(), oi.nmasks
    ok = (C.c_uint64 * M)()
    ooff, olocs = C.POINTER(C.c_int)(), C.POINTER(C.c_int)()
    assert L.lmo_stage_mask(oi.h, seq, len(seq), ok, C.byref(ooff), C.byref(olocs)) == 0
    anc = C.POINTER(O.Anchor)()
    na = L.lmo_stage_anchors(oi.h, ok, ooff, olocs, C.byref(anc))
    out = np.zeros(0, dtype=ANCHOR_DTYPE)
    if na:
        out = np.frombuffer((C.c_char * (na * ANCHOR_DTYPE.itemsize)).from_address(C.addressof(anc.contents)),
                            dtype=ANCHOR_DTYPE).copy()
    L.free(anc)
    L.free(ooff)
    L.free(olocs)
    return out


def rows(a):
    """anchors as an [n, 5] int64 array of (qbegin, tbegin, len, qrc, trc)"""
    return np.stack([a[f].astype(np.int64) for f in FIELDS], axis=1) if len(a) else np.zeros((0, 5), dtype=np.int64)


def split_pairs(a):
    """{genome key: [n, 5] rows} of anchors sorted by genome"""
    out = {}
    if len(a):
        g = a["genome"]
        cut = np.flatnonzero(g[1:] != g[:-1]) + 1
        for part in np.split(np.arange(len(a)), cut):
            out[int(g[part[0]])] = rows(a[part])
    return out


MAX_GAP, MAX_DISTANCE = 50.0, 1000.0  # the defaults of --seed-max-gap / --seed-max-dist


def oracle_chain(raw, k, min_single_prefix=17, max_gap=MAX_GAP, max_distance=MAX_DISTANCE):
    """lmo_clear_subs + lmo_chainer over one pair's raw rows: (cleared rows, score, chains)"""
    import ctypes as C
    L = O.lib()
    n = len(raw)
    subs = (O.Sub * n)()
    v = np.frombuffer(subs, dtype=SUB_DTYPE)
    v["qbegin"], v["tbegin"], v["len"], v["qrc"], v["trc"] = raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3], raw[:, 4]
    nn = L.lmo_clear_subs(subs, n, k) if n > 1 else n
    cleared = np.stack([v[f][:nn].astype(np.int64) for f in FIELDS], axis=1)
    coff, cidx, nch = C.POINTER(C.c_int)(), C.POINTER(C.c_int)(), C.c_int()
    sc = L.lmo_chainer(subs, nn, max_gap, L.lmo_seed_weight(float(min_single_prefix & 255)), max_distance, 0, C.byref(coff),
                       C.byref(cidx), C.byref(nch))
    chains = [[cidx[x] for x in range(coff[c], coff[c + 1])] for c in range(nch.value)]
    L.free(coff)
    L.free(cidx)
    return cleared, sc, chains


# name -> (genomes, oracle build options)
INDEXES = {
    "V20k": (lambda: tiny_genomes(7, 150), dict(chunks=2)),
    "V2k": (lambda: tiny_genomes(7, 150), dict(chunks=2, masks=2000)),
    "C2k": (lambda: copy_genomes(17), dict(chunks=2, masks=2000)),
    "K21": (lambda: tiny_genomes(27, 20), dict(chunks=2, masks=2000, k=21)),
}

_genomes = {}


def genomes_of(name):
    if name not in _genomes:
        _genomes[name] = INDEXES[name][0]()
    return _genomes[name]


def build(name, outdir):
    """the index `name` written by the oracle into outdir/<name>.lmi; returns (path, genomes)"""
    d = os.path.join(outdir, name + ".lmi")
    O.build_index(d, genomes_of(name), O.default_build_opt(**INDEXES[name][1]))
    return d, genomes_of(name)


def genome_key(i):
    """batch << 17 | index of the i-th genome added (one batch here)"""
    return i


# ---- chaining: windows (start, length) of the large genome of V20k whose pair with that genome holds exactly `raw` seed
# anchors before ClearSubstrPairs, on either side of LM_CHAIN1_WAVE_MIN = 48, of the 64-lane chunks of k_chain1_wave and of the
# powers of two its bitonic network pads to.  Found by scan() below; never re-scanned by a test.
CHAIN_TARGETS = (47, 48, 49, 50, 63, 64, 65, 127, 128, 129)
CHAIN_WINDOWS = {47: (4000, 183), 48: (40000, 189), 49: (4000, 184), 50: (40000, 196), 63: (4000, 205), 64: (40000, 270),
                 65: (4000, 208), 127: (40000, 453), 128: (5000, 482), 129: (40000, 457)}
CHAIN_MID = (5000, 1027)  # a window whose pair holds 300 raw anchors


def scan(index_dir, big, targets=CHAIN_TARGETS, starts=(5000, 40000, 77000), lengths=range(150, 1500)):
    """run by hand when the genomes change: windows of `big` whose largest pair has exactly a targeted raw anchor count"""
    oi = O.Index(index_dir)
    found, mid = {}, None
    for ln in lengths:
        for st in starts:
            a = oracle_anchors(oi, big[st:st + ln])
            n = int(np.unique(a["genome"], return_counts=True)[1].max()) if len(a) else 0
            if n in targets and n not in found:
                found[n] = (st, ln)
            if mid is None and 300 <= n <= 500:
                mid = (st, ln)
        if len(found) == len(targets) and mid:
            break
    oi.close()
    return found, mid


def invert_middle(s):
    """s with its middle third reverse-complemented: the chain direction changes inside the pair"""
    a, b = len(s) // 3, 2 * len(s) // 3
    return s[:a] + revcomp(s[a:b]) + s[b:]


def repeat_block(block, rng):
    """a 400-base block three times between random spacers: every captured k-mer of it has three query locations"""
    return random_seq(rng, 60) + block + random_seq(rng, 45) + block + random_seq(rng, 70) + block + random_seq(rng, 30)


def queries(name):
    """[(query name, sequence)] searched in index `name` as ONE batch"""
    g = genomes_of(name)
    big = g[0][1][0][1]
    tiny = [x[1][0][1] for x in g[1:]]
    rng = random.Random(1000 + len(name) + len(g))
    qs = []
    if name == "V20k":
        for t in CHAIN_TARGETS:
            st, ln = CHAIN_WINDOWS[t]
            qs.append(("pair%d" % t, big[st:st + ln]))
        for t in (65, 129):
            st, ln = CHAIN_WINDOWS[t]
            qs.append(("pair%d_rc" % t, revcomp(big[st:st + ln])))
        st, ln = CHAIN_MID
        qs.append(("pair_mid", big[st:st + ln]))
        qs.append(("inverted_middle", invert_middle(big[20000:21800])))
        qs.append(("big_3k", big[9000:12000]))
        i1k = min(range(len(tiny)), key=lambda i: abs(len(tiny[i]) - 1000))
        qs.append(("tiny_1k_whole", tiny[i1k]))
        qs.append(("tiny_window", tiny[3][50:450]))
        qs.append(("tiny_window_rc", revcomp(tiny[8][20:320])))
        qs.append(("block_x3", repeat_block(big[60000:60400], rng)))
    elif name == "V2k":
        for st in range(0, 110000, 9000):
            qs.append(("big_3k_%d" % st, big[st:st + 3000]))
        qs.append(("big_3k_rc", revcomp(big[50000:53000])))
        for i in (0, 5, 17, 40, 99, 149):
            qs.append(("tiny%d_whole" % i, tiny[i]))
        qs.append(("tiny5_rc", revcomp(tiny[5])))
        qs.append(("tiny_window", tiny[3][50:450]))
        qs.append(("inverted_middle", invert_middle(big[20000:23000])))
        qs.append(("block_x3", repeat_block(big[60000:60400], rng)))
        qs.append(("tiny_block_x3", repeat_block((tiny[40] * 3)[:400], rng)))
    elif name == "C2k":
        qs.append(("copy0_whole", tiny[0]))
        qs.append(("copy7_rc", revcomp(tiny[7])))
        qs.append(("copy_window", tiny[3][200:900]))
        qs.append(("copy_block_x3", repeat_block(tiny[1][300:700], rng)))
        qs.append(("big_3k", big[30000:33000]))
    elif name == "K21":
        for st in (0, 40000, 90000):
            qs.append(("big_2k_%d" % st, big[st:st + 2000]))
        for i in (0, 7, 19):
            qs.append(("tiny%d_whole" % i, tiny[i]))
        qs.append(("tiny7_rc", revcomp(tiny[7])))
        qs.append(("block_x3", repeat_block(big[60000:60400], rng)))
    else:
        raise KeyError(name)
    k = INDEXES[name][1].get("k", 31)
    qs.insert(2, ("too_short", big[100:100 + k - 1]))
    qs.insert(4, ("all_N", b"N" * 200))
    return qs


def option_sets(k, p_plus_a):
    """search options by name: the defaults, -p at its lower bound, and -p = -P = k"""
    return {"default": {}, "p_lo": dict(min_prefix=p_plus_a), "p_k": dict(min_prefix=k, min_single_prefix=k)}


class Case:
    """one index with its query batch and, per option set (computed once, on first use), what the oracle and the plain
    model make of every query"""

    def __init__(self, name, outdir):
        import seed_model as SM
        self.name = name
        self.dir, self.genomes = build(name, outdir)
        qs = queries(name)
        self.names, self.seqs = [q[0] for q in qs], [q[1] for q in qs]
        oi = O.Index(self.dir)
        self.M = oi.nmasks
        mp = O.lib().lmo_index_masks(oi.h)
        self.lists = SM.Lists(self.dir, [mp[i] for i in range(self.M)])
        oi.close()
        self.k = self.lists.k
        self.lo = self.lists.p + self.lists.a
        self.options = option_sets(self.k, self.lo)
        self._sets, self._chained, self._captures, self._lookups = {}, {}, None, None

    def set(self, oname):
        """dict(kw, min_prefix, min_single_prefix, oracle: per query {genome: raw rows in ClearSubstrPairs order},
        model: per query {genome: sorted raw rows}, facts)"""
        import seed_model as SM
        if oname not in self._sets:
            kw = self.options[oname]
            oi = O.Index(self.dir, O.default_search_opt(**kw))
            if self._captures is None:  # (masking does not depend on the search options)
                none = (np.zeros(self.M, np.uint64), np.zeros(self.M + 1, np.int64), np.zeros(0, np.int64))
                self._captures = [stage_mask(oi, s) if len(s) >= self.k else none for s in self.seqs]
                self._lookups = SM.issue(self.lists, self._captures)
            oracle = [split_pairs(oracle_anchors(oi, s, self.k)) for s in self.seqs]
            model, facts = SM.search(self.lists, self._captures, oi.opt.min_prefix, lookups=self._lookups)
            self._sets[oname] = dict(kw=kw, min_prefix=oi.opt.min_prefix, min_single_prefix=oi.opt.min_single_prefix,
                                     oracle=oracle, model=model, facts=facts)
            oi.close()
        return self._sets[oname]

    def chained(self, oname):
        """per query {genome: (raw, cleared, score, chains)}: the oracle's ClearSubstrPairs and Chainer.Chain over its own raw
        anchors, at the default --seed-max-gap / --seed-max-dist"""
        if oname not in self._chained:
            s = self.set(oname)
            self._chained[oname] = [{g: (raw,) + oracle_chain(raw, self.k, s["min_single_prefix"], MAX_GAP, MAX_DISTANCE)
                                     for g, raw in per.items()} for per in s["oracle"]]
        return self._chained[oname]

    def model_kept(self, oname, keep):
        """the model's anchors under a genome whitelist"""
        import seed_model as SM
        return SM.search(self.lists, self._captures, self.set(oname)["min_prefix"], keep=set(keep), lookups=self._lookups)[0]
