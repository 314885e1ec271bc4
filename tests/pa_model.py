"""The raw pseudo-alignment anchors of one chain window in plain Python / numpy: what SeqComparator.Index + Compare
(lib-seq_compare.go:115-159, :335-445) append to `subs` before ClearSubstrPairs, restated from the reference.  Shares no code
with lexicmap_amd/csrc/.  TEST INFRASTRUCTURE ONLY.

Inputs: the query bytes, the window TEXT (already turned round for a reverse-strand window), the query range [qbegin, qend].

  * index: every K-mer (K = 31) of the query with its reverse complement, except the positions Index drops - the k-mer is
    AAA.., CCC.., GGG.., TTT.. or low-complexity by DUST.  A non-ACGT byte is no reason to drop a k-mer: the reference's base
    table reads it as a base (B, S, Y -> C; K -> G; everything else, N included -> A), and so does this model.  A query of
    N only therefore indexes nothing (all its k-mers are AAA..).
  * p: 11, +2 / +4 / +6 / +8 for windows of >= 10 000 / 50 000 / 250 000 / 1 000 000 bases.
  * normal rule: at every window position whose k-mer is no homopolymer, for the k-mer and for its reverse complement, every
    indexed k-mer that shares at least p leading bases gives an anchor of the length of the common prefix, subject to the
    range test of Compare.  `plain_matches` finds them by equality of the first p bases over ALL indexed k-mers (a sort
    and two binary searches per position; `brute_matches` is the literal double loop, used on the small cases to pin it).
  * partial-prefix rule (tree.go:496-500): the reference's radix tree also answers some searches in which NO k-mer shares p
    bases, because its check of a partly matching node is done in uint8 arithmetic that wraps.  These matches (shorter than
    p: "quirk" anchors) cannot be stated without the tree, so they come from the oracle's literal tree (lmo_tree_search),
    which is restated from tree.go and pinned by the reference's own test vectors.  The tree is ALSO asked wherever the
    normal rule matches, and must then return exactly the plain form's matches: that pins this model to the oracle.
    The tree is asked at every (position, strand) of windows up to TREE_EVERYWHERE positions.  In longer windows it is asked
    where the plain form matches and where bases p-2 and p-1 of the key are both A: a search without a k-mer sharing p bases
    ends at a node whose edge differs from the key; it is accepted only if the `atleast` = p - matched >= 2 next bases of the key
    equal 0 after the wrapped shift turned the node's side into 0, i.e. are all A (an edge of one base that differs has atleast
    >= 2 as well, since an edge that covers the rest up to p and agrees on it is the normal rule).
  * sort key and clear: ClearSubstrPairs order (QBegin asc, QEnd desc, TBegin asc, QRC, TRC); anchor v is dropped iff an anchor c
    sorting earlier has c.qbegin >= max(0, v.qend - K), v.qend <= c.qend, v.tbegin >= c.tbegin, v.tend <= c.tend (containers are
    taken from the raw list, strands are not compared).

Anchors are tuples (qbegin, tbegin, len, trc, qrc) in window coordinates."""
import ctypes as C

import numpy as np

K = 31
TREE_EVERYWHERE = 6000

_B2 = np.zeros(256, np.uint8)
for _c, _v in (("A", 0), ("C", 1), ("G", 2), ("T", 3), ("U", 3), ("B", 1), ("S", 1), ("Y", 1), ("K", 2)):
    _B2[ord(_c)] = _v
    _B2[ord(_c.lower())] = _v
_MASK = (1 << (2 * K)) - 1
_HOMO = tuple(sum(b << (2 * i) for i in range(K)) for b in range(4))


def min_prefix(wlen, base=11):
    if wlen >= 1000000:
        return base + 8
    if wlen >= 250000:
        return base + 6
    if wlen >= 50000:
        return base + 4
    if wlen >= 10000:
        return base + 2
    return base


def revcomp_text(s):
    return bytes(s)[::-1].translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))


def kmers(seq):
    """(forward, reverse-complement) K-mers of every position, uint64"""
    c = _B2[np.frombuffer(bytes(seq), np.uint8)].astype(np.uint64)
    n = len(c) - K + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    f = np.zeros(n, np.uint64)
    r = np.zeros(n, np.uint64)
    for j in range(K):
        f = (f << np.uint64(2)) | c[j:j + n]
        r = r | ((np.uint64(3) - c[j:j + n]) << np.uint64(2 * j))
    return f, r


def dust(f):
    """util/kmers.go:162-328 for an array of K-mers: the 3-base windows at bit shifts 0, 2, .., 2(K-2) (the last reaches two zero
    bits above the k-mer); score = sum over the distinct windows of c(c-1)/2 = the number of equal pairs; low complexity: > 50"""
    t = [(f >> np.uint64(2 * i)) & np.uint64(63) for i in range(K - 1)]
    score = np.zeros(len(f), np.int32)
    for i in range(len(t)):
        for j in range(i + 1, len(t)):
            score += t[i] == t[j]
    return score > 50


def lcp(a, b):
    x = int(a) ^ int(b)
    return K if x == 0 else K - ((x.bit_length() + 1) >> 1)


class QueryIndex:
    """SeqComparator.Index: sorted (k-mer, position << 1 | strand) of both strands of every kept position"""

    def __init__(self, q):
        self.q = bytes(q)
        f, r = kmers(self.q)
        keep = np.ones(len(f), bool)
        for h in _HOMO:
            keep &= f != np.uint64(h)
        if len(f):
            keep &= ~dust(f)
        pos = np.nonzero(keep)[0].astype(np.uint64)
        keys = np.concatenate([f[keep], r[keep]])
        vals = np.concatenate([pos << np.uint64(1), (pos << np.uint64(1)) | np.uint64(1)])
        o = np.argsort(keys, kind="stable")
        self.keys, self.vals = keys[o], vals[o]
        self.npos, self.nkept = len(f), int(keep.sum())
        self._tree = None
        self._pfx = {}

    def prefixes(self, p):
        if p not in self._pfx:
            self._pfx[p] = self.keys >> np.uint64(2 * (K - p))
        return self._pfx[p]

    def tree(self):
        """the oracle's literal radix tree over the same entries"""
        if self._tree is None:
            import oracle as O
            L = O.lib()
            t = L.lmo_tree_new(K)
            for k, v in zip(self.keys.tolist(), self.vals.tolist()):
                L.lmo_tree_insert(t, k, v)
            self._tree = t
        return self._tree

    def close(self):
        if self._tree is not None:
            import oracle as O
            O.lib().lmo_tree_free(self._tree)
            self._tree = None


def tree_matches(qi, key, p):
    """[(k-mer, len_prefix, value)] of lmo_tree_search"""
    import oracle as O
    L = O.lib()
    srs, cap = C.POINTER(O.TreeSr)(), C.c_int(0)
    n = L.lmo_tree_search(qi.tree(), int(key), p, C.byref(srs), C.byref(cap))
    out = []
    for i in range(n):
        for j in range(srs[i].nvals):
            out.append((srs[i].kmer, srs[i].len_prefix, srs[i].vals[j]))
    if cap.value:
        L.free(srs)
    return out


def brute_matches(qi, key, p):
    out = []
    for k, v in zip(qi.keys.tolist(), qi.vals.tolist()):
        lp = lcp(k, key)
        if lp >= p:
            out.append((k, lp, v))
    return out


def _anchor(strand, i, lp, v, qbegin, qend):
    """the range test and the anchor of Compare (lib-seq_compare.go:386-437); None: skipped"""
    if strand == 0:
        qp = v >> 1
        if (v & 1) == 1 or qp < qbegin or qp + lp > qend:
            return None
        return (qp, i, lp, 0, 0)
    qp = (v >> 1) + K - lp
    if (v & 1) == 0 or qp + lp < qbegin or qp > qend:
        return None
    return (qp, i + K - lp, lp, 1, 1)


def sort_key(a):
    return (a[0], -(a[0] + a[2]), a[1], a[4], a[3])


def clear(anchors):
    """ClearSubstrPairs of a list in any order: the kept anchors, sorted"""
    s = sorted(anchors, key=sort_key)
    if len(s) < 2:
        return s
    qb = np.array([a[0] for a in s], np.int64)
    tb = np.array([a[1] for a in s], np.int64)
    ln = np.array([a[2] for a in s], np.int64)
    qe, te = qb + ln, tb + ln
    out = [s[0]]
    for i in range(1, len(s)):
        lo = int(np.searchsorted(qb[:i], max(0, int(qe[i]) - K), "left"))
        if lo < i and bool(np.any((qe[i] <= qe[lo:i]) & (tb[i] >= tb[lo:i]) & (te[i] <= te[lo:i]))):
            continue
        out.append(s[i])
    return out


class Result:
    def __init__(self):
        self.raw = []            # anchors, unsorted
        self.owners = set()      # (window position, strand) that own an anchor
        self.matches = {}        # (window position, strand) -> sorted [(k-mer, len, value)] before the range test
        self.p = 0
        self.counters = dict(raw=0, quirk=0, fwd=0, rev=0, multi=0, cleared=0, removed=0, tree_calls=0, tree_checked=0)


def model(qi, window, qbegin, qend, brute=False):
    """raw anchors of one window; asserts that the tree form equals the plain form wherever the plain form matches"""
    window = bytes(window)
    res = Result()
    p = res.p = min(min_prefix(len(window)), K)
    f, r = kmers(window)
    n = len(f)
    if n == 0 or len(qi.keys) == 0:
        return res
    live = np.ones(n, bool)
    for h in _HOMO:
        live &= f != np.uint64(h)
    kp = qi.prefixes(p)
    every = n <= TREE_EVERYWHERE
    cnt = res.counters
    sh = np.uint64(2 * (K - p))
    for strand, keys in ((0, f), (1, r)):
        pf = keys >> sh
        lo = np.searchsorted(kp, pf, "left")
        hi = np.searchsorted(kp, pf, "right")
        has = live & (hi > lo)
        aa = live & ((pf & np.uint64(15)) == 0)
        ask = live if every else (has | aa)
        for i in np.nonzero(ask)[0].tolist():
            key = int(keys[i])
            plain = sorted((int(qi.keys[j]), lcp(qi.keys[j], key), int(qi.vals[j])) for j in range(int(lo[i]), int(hi[i])))
            if brute:
                assert plain == sorted(brute_matches(qi, key, p)), "plain form differs from the double loop at %d/%d" % (i, strand)
            tree = sorted(tree_matches(qi, key, p))
            cnt["tree_calls"] += 1
            if plain:
                cnt["tree_checked"] += 1
                assert tree == plain, "tree form differs from the plain form at window position %d strand %d: %r vs %r" % (
                    i, strand, tree[:4], plain[:4])
            elif tree:
                assert every or bool(aa[i])
                assert all(m[1] < p for m in tree), "a tree match of >= p bases that the plain form misses"
            if not bool(aa[i]) and not plain:
                assert not tree, "the tree answers a search whose bases p-2, p-1 are not AA and that shares p bases with nothing"
            if not tree:
                continue
            res.matches[(i, strand)] = tree
            got = 0
            for _, lp, v in tree:
                a = _anchor(strand, i, lp, v, qbegin, qend)
                if a is None:
                    continue
                res.raw.append(a)
                got += 1
                cnt["quirk"] += lp < p
                cnt["rev" if strand else "fwd"] += 1
            if got:
                res.owners.add((i, strand))
            cnt["multi"] += got > 1
    cnt["raw"] = len(res.raw)
    return res
