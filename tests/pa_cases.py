"""Named edge cases of the pseudo-alignment anchor stage (k_pa_filter + k_pa_search): windows of a few small genomes, chosen by
where the kernels change path - word offsets of the 2-bit genome, lane / slice boundaries of the rolling and of the strided
filter, the window-length classes of the minimum prefix, the query's filter class, task groups and runs, the staging strips,
the partial-prefix rule of the radix tree and the range test of Compare.  TEST INFRASTRUCTURE ONLY (tests/pa_model.py says
what every case must give; test_pa_edges_cpu.py and test_gpu_pa_edges.py run them).

A case is a window of one genome in one orientation, compared with one query over a query range.  Most cases plant exact
copies of query stretches into a window of unrelated random bases, with a mismatching base on each side, so that a copy
of m bases gives exactly the anchors of an exact run of m bases.  Every family comes in both window orientations: for
rc = 1 the genome holds the reverse complement of the window text.

build() is deterministic; it returns the genomes (input of Index.from_genomes), the queries, the cases and the calls (lists of
case numbers that go to the library in one call; "main" holds every case once except the two of "many", which have their own)."""
import random
from collections import namedtuple

import pa_model as M

K = 31
Case = namedtuple("Case", "name family q qbegin qend g tbegin wlen rc plants")
# plants: [(m, query position, window position)] of the forward copies planted into this window's text

# how many cases of each family the suite must reach (check_reached asserts these and, from the model's counters, that every
# family has anchors, every partial-prefix case an anchor of that rule and the tandem repeats their tens of thousands)
FAMILIES = {
    "align": 72,        # tbegin mod 32 x (tbegin + wlen) mod 32, each in {0, 1, 15, 16, 17, 31}, x 2 orientations
    "store_edges": 4,   # first genome of the store from base 0, last genome up to its last base
    "wlen": 20,         # 30, 31, 32, 94, 95, 1950, 1951, 2078, 2079, 4127
    "pclass": 12,       # 9 999 / 10 000, 49 999 / 50 000, 249 999 / 250 000
    "qclass": 12,       # queries of 30, 31, 8 191, 8 192, 16 414, 16 415 bases
    "qcontent": 8,      # non-ACGT bytes, all N, homopolymer runs, a k-mer that occurs three times
    "many": 2,          # tandem repeats of period 7
    "partial": 12,      # partial-prefix rule, p = 11, 13, 15, short and long query
    "range": 16,        # the range test of Compare at qbegin - 1, qbegin, qend, qend + 1
    "groups": 10,       # three queries in one group, an empty window and an all-N query between ordinary ones
    "pending": 6,       # a query above 16 414 bases against windows with p = 11, 13, 15: ordinary copies through the pending list
}
ALIGN = (0, 1, 15, 16, 17, 31)
PLANT_LENS = lambda p: (p - 1, p, p + 1, 31, 32, 40)


def rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


_COMP = {65: 84, 67: 71, 71: 67, 84: 65}


def _other(rng, b):
    return rng.choice([c for c in b"ACGT" if c != b])


def filter_slices(npos, roll):
    """[(p0, p1, positions per lane)] of a window of npos positions, as k_pa_filter cuts it: the rolling form in equal slices of at
    most 2048 positions with ceil(np / 64) consecutive positions per lane, the strided form in slices of 1920"""
    if npos <= 0:
        return []
    if roll:
        ns = (npos + 2047) // 2048
        sl = (npos + ns - 1) // ns
    else:
        ns, sl = (npos + 1919) // 1920, 1920
    out = []
    for s in range(ns):
        p0, p1 = s * sl, min(s * sl + sl, npos)
        out.append((p0, p1, (p1 - p0 + 63) >> 6 if roll else 1))
    return out


def boundaries(npos, rc):
    """[(kind, x)]: the window positions x, x + 1 lie on either side of a hand-over of k_pa_filter.  A slice is a range [p0, p1) of
    window positions in either orientation, so "slice_roll" / "slice_strided" are x = p1 - 1 for every slice but the last.  Inside a
    rolling slice lane l holds the slice positions [bpl l, bpl (l + 1)) in GENOME order, which a reverse-strand window walks
    backwards (slice position r is window position p1 - 1 - r): "lane" names the first, a middle and the last lane boundary of
    every rolling slice"""
    out = []
    for roll in (True, False):
        for p0, p1, bpl in filter_slices(npos, roll):
            if p1 < npos:
                out.append(("slice_roll" if roll else "slice_strided", p1 - 1))
            if roll:
                lanes = (p1 - p0 + bpl - 1) // bpl
                for l in sorted({1, lanes // 2, lanes - 1}):
                    if 1 <= l < lanes:
                        out.append(("lane", p1 - 1 - bpl * l if rc else p0 + bpl * l - 1))
    return sorted(set(out), key=lambda t: (t[1], t[0]))


def boundary_plants(npos, rc, qlen):
    """copies that put a k-mer with >= 31 common bases on both sides of every boundary: one copy of 40 bases from x - 4 for a boundary
    on its own, one longer copy over boundaries less than 60 positions apart"""
    xs = sorted({x for _, x in boundaries(npos, rc)})
    groups = []
    for x in xs:
        if groups and x - groups[-1][-1] < 60:
            groups[-1].append(x)
        else:
            groups.append([x])
    out = []
    for j, g in enumerate(groups):
        wp = max(g[0] - 4, 0)
        m = min(g[-1] + 1 + 35, npos + K - 1) - wp   # (clipped at the window's last base)
        assert m + 20 < qlen
        out.append((m, 20 + 37 * j % (qlen - m - 20), wp))
    return out


class _Builder:
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.genomes = []   # [name, bytearray]
        self.queries = []
        self.cases = []

    def query(self, seq):
        self.queries.append(bytes(seq))
        return len(self.queries) - 1

    def genome(self, name):
        self.genomes.append([name, bytearray()])
        return len(self.genomes) - 1

    def window_text(self, q, wlen, plants, fill=None):
        """wlen unrelated bases with q[qp : qp + m] copied to wp for every (m, qp, wp), a mismatching base on each side"""
        rng = self.rng
        w = bytearray(fill if fill is not None else rand(rng, wlen))
        qs = self.queries[q]
        for m, qp, wp in plants:
            assert 0 <= qp and qp + m <= len(qs) and 0 <= wp and wp + m <= wlen, (m, qp, wp, wlen)
            w[wp:wp + m] = qs[qp:qp + m]
        for m, qp, wp in plants:  # (after all copies: a flank never lands inside another copy by construction of the callers)
            if wp > 0 and qp > 0:
                w[wp - 1] = _other(rng, qs[qp - 1])
            if wp + m < wlen and qp + m < len(qs):
                w[wp + m] = _other(rng, qs[qp + m])
        return bytes(w)

    def place(self, g, text, rc, mod=None):
        """appends the window (its reverse complement for rc) to genome g at an offset with tbegin mod 32 == mod"""
        buf = self.genomes[g][1]
        if mod is not None:
            while len(buf) % 32 != mod:
                buf += rand(self.rng, 1)
        tb = len(buf)
        buf += M.revcomp_text(text) if rc else text
        return tb

    def case(self, name, family, q, g, tbegin, wlen, rc, plants=(), qbegin=0, qend=None):
        qend = len(self.queries[q]) - 1 if qend is None else qend
        self.cases.append(Case(name, family, q, qbegin, max(qend, 0), g, tbegin, wlen, rc, tuple(plants)))
        return len(self.cases) - 1

    def planted(self, name, family, q, g, wlen, rc, plants, mod=None, **kw):
        text = self.window_text(q, wlen, plants)
        tb = self.place(g, text, rc, mod)
        return self.case(name, family, q, g, tb, wlen, rc, plants, **kw)


def build(seed=20250921):
    b = _Builder(seed)
    rng = b.rng
    calls = {}
    q0 = b.query(rand(rng, 600))
    g_first, g_mid = b.genome("PA_first"), b.genome("PA_mid")

    # ---- store edges, part 1: the first genome of the store from its base 0 (and, below, the last one up to its last base); both
    # orientations read the same bases, so the copies at the ends are a match at window position 0 and one at the last position
    pl = [(31, 100, 0), (40, 200, 150), (31, 300, 269)]
    tb = b.place(g_first, b.window_text(q0, 300, pl), 0)
    assert tb == 0
    b.case("first_genome_base0_rc0", "store_edges", q0, g_first, 0, 300, 0, pl)
    b.case("first_genome_base0_rc1", "store_edges", q0, g_first, 0, 300, 1)
    b.genomes[g_first][1] += rand(rng, 700)

    # ---- word alignment: a match at window position 0, one at the last position, one of a varying length between
    n = 0
    for a in ALIGN:
        for e in ALIGN:
            for rc in (0, 1):
                wlen = 224 + ((e - a - 224) % 32)
                mid = PLANT_LENS(11)[n % 6]
                n += 1
                i = b.planted("align_%d_%d_rc%d" % (a, e, rc), "align", q0, g_mid, wlen, rc,
                              [(31, 50, 0), (mid, 150, 100), (31, 250, wlen - 31)], mod=a)
                c = b.cases[i]
                assert c.tbegin % 32 == a and (c.tbegin + c.wlen) % 32 == e

    # ---- window lengths: no position, one, two; 64 / 65 positions; one / two slices of either form; three slices.  Copies straddle
    # every slice boundary of both forms and the first, a middle and the last lane boundary of every rolling slice (boundaries());
    # a copy of 150 bases, in the first stretch free of them, gives a chain
    for wlen in (30, 31, 32, 94, 95, 1950, 1951, 2078, 2079, 4127):
        for rc in (0, 1):
            npos = wlen - K + 1
            plants = []
            if wlen == 31:
                plants = [(31, 77, 0)]
            elif wlen == 32:
                plants = [(32, 77, 0)]
            elif wlen in (94, 95):
                plants = [(40, 77, 10), (31, 300, wlen - 31)]
            elif wlen > 95:
                plants = boundary_plants(npos, rc, len(b.queries[q0]))
                free = 40
                for m, _, wp in plants:
                    if wp - free >= 230:
                        break
                    free = max(free, wp + m + 40)
                assert free + 190 < wlen
                plants = [(150, 400, free + 20)] + plants
            b.planted("wlen_%d_rc%d" % (wlen, rc), "wlen", q0, g_mid, wlen, rc, plants, mod=(wlen * 7 + rc) % 32)

    # ---- length classes of p: nested windows [0, L) of one 250 000-base genome; copies of every boundary length, forward and
    # reverse-complemented in the genome, so that both orientations read forward copies
    g_big = b.genome("PA_big")
    lens = sorted({m for p in (11, 13, 15, 17) for m in PLANT_LENS(p)})
    big = bytearray(rand(rng, 250000))
    qs = b.queries[q0]
    fwd_plants, rev_plants = [], []
    for n, m in enumerate(lens):
        qp, gp = 20 + 41 * n, 500 + 200 * n
        fwd_plants.append((m, qp, gp))
        gp2 = 5000 + 200 * n
        rev_plants.append((m, qp, gp2))
    for m, qp, gp in fwd_plants:
        big[gp:gp + m] = qs[qp:qp + m]
        big[gp - 1], big[gp + m] = _other(rng, qs[qp - 1]), _other(rng, qs[qp + m])
    for m, qp, gp in rev_plants:
        big[gp:gp + m] = M.revcomp_text(qs[qp:qp + m])
        big[gp + m], big[gp - 1] = _other(rng, _COMP[qs[qp - 1]]), _other(rng, _COMP[qs[qp + m]])
    b.genomes[g_big][1] += big
    for L in (9999, 10000, 49999, 50000, 249999, 250000):
        for rc in (0, 1):
            if rc == 0:
                plants = fwd_plants
            else:  # the reverse-complemented copies read forward: genome [gp, gp + m) is window [L - gp - m, L - gp)
                plants = [(m, qp, L - gp - m) for m, qp, gp in rev_plants]
            b.case("pclass_%d_rc%d" % (L, rc), "pclass", q0, g_big, 0, L, rc, plants)

    # ---- query classes: nothing indexed, one k-mer, by-group candidate segments from 8192 bases, the LDS Bloom filter alone up to
    # 16 414 bases and the pending list + the global bitmap beyond; the copies come from the end of the query
    g_q = b.genome("PA_query_classes")
    qclass = {}
    for qlen in (30, 31, 8191, 8192, 16414, 16415):
        qi = qclass[qlen] = b.query(rand(rng, qlen))
        for rc in (0, 1):
            if qlen == 30:
                plants = []
            elif qlen == 31:
                plants = [(31, 0, 100)]
            else:
                plants = [(m, qlen - 80 * (j + 1), 60 + 80 * j) for j, m in enumerate(PLANT_LENS(11))]
            # (qend = 31 for the query of 31 bases: with the usual last index, 30, Compare skips the one forward anchor, 0 + 31 > 30)
            b.planted("qlen_%d_rc%d" % (qlen, rc), "qclass", qi, g_q, 700, rc, plants, mod=(qlen + 5 * rc) % 32, qend=31 if qlen == 31 else None)

    # ---- query content
    qn = bytearray(rand(rng, 500))
    qn[119], qn[160], qn[175], qn[300] = ord("N"), ord("N"), ord("R"), ord("n")   # next to, and inside, the copied stretches
    q_n = b.query(bytes(qn))
    q_alln = b.query(b"N" * 200)
    qh = bytearray(rand(rng, 500))
    qh[100:150], qh[250:290], qh[330:380] = b"A" * 50, b"C" * 40, b"AT" * 25
    q_h = b.query(bytes(qh))
    rep = rand(rng, 45)
    q_3 = b.query(rand(rng, 100) + rep + rand(rng, 80) + rep + rand(rng, 60) + rep + rand(rng, 100))
    for rc in (0, 1):
        b.planted("query_with_N_rc%d" % rc, "qcontent", q_n, g_q, 600, rc, [(40, 120, 50), (40, 150, 200), (40, 290, 350)], mod=3 + rc)
        b.planted("query_all_N_rc%d" % rc, "qcontent", q_alln, g_q, 300, rc, [(40, 10, 50)], mod=9 + rc)
        text = bytearray(b.window_text(q_h, 900, [(70, 90, 50), (60, 240, 200), (70, 320, 350)]))
        text[500:560], text[600:650], text[700:760] = b"A" * 60, b"T" * 50, b"G" * 60                    # homopolymer window k-mers
        tb = b.place(g_q, bytes(text), rc, 20 + rc)
        b.case("homopolymers_rc%d" % rc, "qcontent", q_h, g_q, tb, 900, rc, [(70, 90, 50), (60, 240, 200), (70, 320, 350)])
        b.planted("kmer_three_times_rc%d" % rc, "qcontent", q_3, g_q, 400, rc, [(45, 100, 100)], mod=27 + rc)

    # ---- many anchors: tandem repeats of period 7 in the query and in the window
    unit = b"ACGGTCA"
    q_t = b.query(rand(rng, 30) + unit * 70 + rand(rng, 30))
    for rc in (0, 1):
        text = rand(rng, 40) + unit * 140 + rand(rng, 40)
        tb = b.place(g_q, text, rc, 11 + 6 * rc)
        b.case("tandem7_rc%d" % rc, "many", q_t, g_q, tb, len(text), rc)
    calls["many"] = [len(b.cases) - 2, len(b.cases) - 1]

    # ---- partial-prefix rule: window k-mers X + w7 w8 + A.. (bases [9, p) all A), query k-mers that share exactly 7, 8, 9, 10 bases
    # with them in pairs that share one to three bases more with each other (tree nodes with short edges), sibling 11-base prefixes
    # present / absent; for p = 11, 13, 15, under a short query and under one longer than 16 414 bases
    g_p = b.genome("PA_partial")
    for p, wlen in ((11, 3000), (13, 10000), (15, 50000)):
        wk, qk = [], []
        for n in range(24):
            X = rand(rng, 7)
            w78 = (b"AA", b"CA", b"CG", b"GA")[n % 4]
            tail = rand(rng, K - p)
            wk.append(X + w78 + b"A" * (p - 9) + tail)
            for share in (7, 8, 9, 10):
                if not (n >> (share - 7)) & 1 and n % 5:
                    continue
                stem = wk[-1][:share] + bytes([_other(rng, wk[-1][share])]) + rand(rng, rng.randrange(3))
                qk.append(stem + rand(rng, K - len(stem)))
                qk.append(stem + rand(rng, K - len(stem)))
            if n % 3 == 0:  # a sibling of the 11-base prefix: the same 10 bases, another 11th
                stem = wk[-1][:10] + bytes([_other(rng, wk[-1][10])])
                qk.append(stem + rand(rng, K - 11))
        qseq = b"".join(k + rand(rng, 3) for k in qk)
        q_s = b.query(qseq)
        q_l = b.query(qseq + rand(rng, 16500))
        text = bytearray(rand(rng, wlen))
        for n, k in enumerate(wk):
            at = 100 + (wlen - 300) * n // len(wk)
            text[at:at + K] = k
        for rc in (0, 1):
            tb = b.place(g_p, bytes(text), rc, (p + 13 * rc) % 32)
            b.case("partial_p%d_short_rc%d" % (p, rc), "partial", q_s, g_p, tb, wlen, rc)
            b.case("partial_p%d_long_rc%d" % (p, rc), "partial", q_l, g_p, tb, wlen, rc)

    # ---- range test (lib-seq_compare.go:386, :414): the forward search skips an anchor iff qp < qbegin or qp + len > qend, the reverse
    # search (which sees the copies of the query's reverse complement) iff qp + len < qbegin or qp > qend; the full-length anchors of
    # the copies of query [100, 140) and [300, 340) sit on either side of each of the four bounds
    g_r = b.genome("PA_range")
    for rc in (0, 1):
        text = bytearray(b.window_text(q0, 500, [(40, 100, 60), (40, 300, 200)]))
        text[320:360] = M.revcomp_text(qs[100:140])
        text[420:460] = M.revcomp_text(qs[300:340])
        tb = b.place(g_r, bytes(text), rc, 30 - 29 * rc)
        for name, qb_, qe_ in (("qbegin_minus_1", 101, 599), ("qbegin", 100, 599), ("qend_fwd", 0, 140), ("qend_fwd_plus_1", 0, 139),
                               ("rev_qend", 0, 309), ("rev_qend_plus_1", 0, 308), ("rev_qbegin", 131, 599), ("rev_qbegin_minus_1", 132, 599)):
            b.case("range_%s_rc%d" % (name, rc), "range", q0, g_r, tb, 500, rc, [(40, 100, 60), (40, 300, 200)], qbegin=qb_, qend=qe_)

    # ---- groups and runs: windows of three queries of different classes (100 bases, 20 kb, 100 bases) next to each other, a window
    # without a position and a problem of the all-N query between ordinary ones
    q_a, q_b, q_c = b.query(rand(rng, 100)), b.query(rand(rng, 20000)), b.query(rand(rng, 100))
    first = len(b.cases)
    for rc in (0, 1):
        b.planted("group_short_a_rc%d" % rc, "groups", q_a, g_r, 260, rc, [(40, 30, 100)], mod=5)
        b.planted("group_empty_window_rc%d" % rc, "groups", q_a, g_r, 30, rc, [], mod=7)          # between two ordinary problems
        b.planted("group_long_rc%d" % rc, "groups", q_b, g_r, 900, rc, [(m, 19000 + 60 * j, 50 + 120 * j) for j, m in enumerate(PLANT_LENS(11))], mod=18)
        b.planted("group_all_N_rc%d" % rc, "groups", q_alln, g_r, 200, rc, [], mod=12)           # between two ordinary problems
        b.planted("group_short_c_rc%d" % rc, "groups", q_c, g_r, 260, rc, [(40, 50, 130)], mod=31)
    calls["three_queries"] = list(range(first, len(b.cases)))

    # ---- store edges, part 2: the last genome of the store up to its last base
    g_last = b.genome("PA_last")
    b.genomes[g_last][1] += rand(rng, 900)
    pl = [(31, 120, 0), (40, 220, 140), (31, 330, 302)]
    tb = b.place(g_last, b.window_text(q0, 333, pl), 0, 17)
    assert tb + 333 == len(b.genomes[g_last][1])
    b.case("last_genome_last_base_rc0", "store_edges", q0, g_last, tb, 333, 0, pl)
    b.case("last_genome_last_base_rc1", "store_edges", q0, g_last, tb, 333, 1)

    # ---- the pending list at every minimum prefix it carries: a query longer than 16 414 bases (the filter sets the position aside with
    # its first p bases and a 2-bit code of p, and asks the global bitmap 64 positions at a time) against windows of 3 000, 10 000 and
    # 50 000 bases (p = 11, 13, 15) with ordinary copies - a code decoded as another p loses them
    for wlen in (3000, 10000, 50000):
        for rc in (0, 1):
            pp = M.min_prefix(wlen)
            plants = [(m, 16415 - 90 * (j + 1), 500 + (wlen - 1000) * j // 6) for j, m in enumerate(PLANT_LENS(pp))]
            b.planted("pending_p%d_rc%d" % (pp, rc), "pending", qclass[16415], g_p, wlen, rc, plants, mod=(wlen // 1000 + 9 * rc) % 32)

    # ---- calls of 63, 64, 65 and 129 problems (one query: per-wavefront candidate segments), a group boundary inside
    al = [i for i, c in enumerate(b.cases) if c.family == "align"]
    wl = [i for i, c in enumerate(b.cases) if c.family == "wlen"]
    pool = al + wl + al
    for n in (63, 64, 65, 129):
        calls["n%d" % n] = pool[:n]
    # (the tandem repeats go alone, in "many": chaining their ~10^5 anchors per window takes k_pa_chain seconds, which the
    # tests that are not about them need not pay)
    calls["main"] = [i for i, c in enumerate(b.cases) if c.family != "many"]
    genomes = [(name, [(name + "_c", bytes(buf))]) for name, buf in b.genomes]
    return dict(genomes=genomes, queries=b.queries, cases=b.cases, calls=calls)


STORE_TABLE = bytearray(b"A" * 256)   # the 2-bit table of the genome store and back (genome.go:1427-1444)
for _src, _dst in ((b"Aa", b"A"), (b"CcBbSsYy", b"C"), (b"GgKk", b"G"), (b"TtUu", b"T")):
    for _c in _src:
        STORE_TABLE[_c] = _dst[0]
STORE_TABLE = bytes(STORE_TABLE)


def window_text(fx, c):
    """the window of case c as text: from fx["fetched"] (the genomes as the library returns them) when that is there, else from the
    input genomes under the store's base table"""
    g = fx["fetched"][c.g] if "fetched" in fx else fx["genomes"][c.g][1][0][1].translate(STORE_TABLE)
    t = g[c.tbegin:c.tbegin + c.wlen]
    return M.revcomp_text(t) if c.rc else t


def run_models(fx, brute_below=0):
    """{case number: pa_model.Result} with .cleared and .text added; one QueryIndex per query (kept in fx["qindex"]).  brute_below:
    cases whose window has fewer positions and whose query has fewer than 1500 indexed k-mers also run the literal double loop"""
    qi = fx.setdefault("qindex", {})
    out = {}
    for n, c in enumerate(fx["cases"]):
        if c.q not in qi:
            qi[c.q] = M.QueryIndex(fx["queries"][c.q])
        text = window_text(fx, c)
        r = M.model(qi[c.q], text, c.qbegin, c.qend, brute=len(text) - K + 1 < brute_below and len(qi[c.q].keys) < 1500)
        r.text = text
        r.sorted = sorted(r.raw, key=M.sort_key)
        r.cleared = M.clear(r.sorted)
        r.counters["cleared"] = len(r.cleared)
        r.counters["removed"] = len(r.raw) - len(r.cleared)
        out[n] = r
    return out


def family_totals(fx, res):
    fam = {}
    for n, c in enumerate(fx["cases"]):
        d = fam.setdefault(c.family, dict(cases=0))
        d["cases"] += 1
        for k, v in res[n].counters.items():
            d[k] = d.get(k, 0) + v
    return fam


def check_reached(fx, res):
    """the reached counters of the suite, from the model alone: every family with its stated number of cases and with anchors, quirk
    anchors at every p of the partial-prefix family under both query classes, both strands, multi-match positions, anchors that
    ClearSubstrPairs removes"""
    fam = family_totals(fx, res)
    assert {f: d["cases"] for f, d in fam.items()} == FAMILIES
    for f, d in fam.items():
        assert d["raw"] > 0, "family %s has no anchor" % f
    tot = {k: sum(d.get(k, 0) for d in fam.values()) for k in ("raw", "quirk", "fwd", "rev", "multi", "removed")}
    for k, v in tot.items():
        assert v > 0, k
    for n, c in enumerate(fx["cases"]):
        if c.family == "partial":
            assert res[n].counters["quirk"] > 0, "no anchor of the partial-prefix rule in %s" % c.name
        if c.family == "many":
            assert res[n].counters["raw"] > 20000 and res[n].counters["multi"] > 500, c.name
    return fam, tot
