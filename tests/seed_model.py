"""A plain statement of the reference's seed lookup and anchor assembly, for the seed-edge tests.  Test infrastructure only.

Written from the reference's Go text (kv/kv-reader.go:762-1021, kv/kv-searcher2.go:105-549, lib-index-search.go:1268-1562);
it shares no code with the product's lm_* or with oracle/lmo_search.c.  Inputs are DATA only: the flat (k-mer, value) list of
every mask as the reference's reader returns it (lmo_kv_load: the lists, not its index) and the captured k-mers and locations
of the queries (lmo_stage_mask: masking has a parity test of its own).

  lookup     of k-mer x in the list of mask m, direction d, at prefix length P: every stored (k, v) with k in
             [x & ~low, x | low], low = 4^(K - P) - 1, and v & 1 == d.  A linear filter over the list; no binary search.
  start rule the reader makes ONE pass over the whole sorted list of a mask (both directions together) and notes, wherever
             the anchor bases (the a bases after the mask's p-base prefix) differ from the k-mer before,
             index[anchor] = position.  A later run of k-mers with the same anchor bases overwrites an earlier one.  The
             searcher starts at index[anchor of the range's left end] and walks upwards, so a lookup whose range lies before
             that position returns nothing.
  reverse    the reversed k-mer is looked up in the list of its arg-min mask (masks sharing its p-base prefix, smallest
             mask XOR k-mer), once per distinct captured k-mer, with the locations of the first mask that captured it.
  anchors    one (qbegin, tbegin, len, qrc, trc) per (returned value, query location); len = common prefix of the looked-up
             and the stored k-mer (lib-index-search.go:1398-1562).
"""
import ctypes as C
import os

import numpy as np

import oracle as O

U = np.uint64


class _KvMem(C.Structure):  # lmo_kv_mem (oracle/lmo.h): the reference's RAM form of a chunk file
    _fields_ = [("k", C.c_int), ("chunk_index", C.c_int), ("chunk_size", C.c_int), ("mask_prefix", C.c_int),
                ("anchor_prefix", C.c_int), ("use7", C.c_int), ("kv", C.POINTER(C.POINTER(C.c_uint64))),
                ("kvlen", C.POINTER(C.c_int64)), ("index", C.POINTER(C.POINTER(C.c_int64)))]


class Lists:
    """the (k-mer, value) lists of every mask of an index directory, and the masks"""

    def __init__(self, index_dir, masks):
        L = O.lib()
        L.lmo_kv_load.restype = C.POINTER(_KvMem)
        L.lmo_kv_load.argtypes = [C.c_char_p]
        L.lmo_kv_free.argtypes = [C.POINTER(_KvMem)]
        self.masks = np.asarray(masks, dtype=U)
        self.keys, self.vals = {}, {}
        for chunk in sorted(os.listdir(os.path.join(index_dir, "seeds"))):
            if not chunk.endswith(".bin"):
                continue
            m = L.lmo_kv_load(os.path.join(index_dir, "seeds", chunk).encode())
            km = m.contents
            self.k, self.p, self.a = km.k, km.mask_prefix, km.anchor_prefix
            for i in range(km.chunk_size):
                n = km.kvlen[i]
                flat = np.ctypeslib.as_array(km.kv[i], shape=(n,)).copy() if n else np.zeros(0, dtype=U)
                self.keys[km.chunk_index + i], self.vals[km.chunk_index + i] = flat[0::2], flat[1::2]
            L.lmo_kv_free(m)
        assert len(self.keys) == len(self.masks)
        for ks in self.keys.values():
            assert (ks[1:] >= ks[:-1]).all()  # what the reader's single pass presumes
        self._index = {}
        self._by_prefix = {}
        for j, pf in enumerate((self.masks >> U(2 * (self.k - self.p))).tolist()):
            self._by_prefix.setdefault(pf, []).append(j)

    def prefix_of(self, x):
        return x >> U(2 * (self.k - self.p))

    def anchor_of(self, x):
        return (x >> U(2 * (self.k - self.p - self.a))) & U(4 ** self.a - 1)

    def start_index(self, m):
        """{anchor: position} after the reader's pass over list m: the last run of an anchor wins"""
        if m not in self._index:
            index, prev = {}, None
            for pos, anc in enumerate(self.anchor_of(self.keys[m]).tolist()):
                if anc != prev:
                    index[anc] = pos
                    prev = anc
            self._index[m] = index
        return self._index[m]

    def argmin_mask(self, x):
        cand = self._by_prefix[int(self.prefix_of(U(x)))]
        h = self.masks[cand] ^ U(x)
        return cand[int(np.argmin(h))]  # (the first of equal minima, as `h < minh` keeps it)


def reverse_kmer(x, k):
    r = 0
    for _ in range(k):
        r = (r << 2) | (x & 3)
        x >>= 2
    return r


def common_prefix(x, y, k):
    """bases shared from the left by the k-mers of two uint64 arrays"""
    n = np.zeros(len(x), dtype=np.int64)
    alive = np.ones(len(x), dtype=bool)
    for i in range(1, k + 1):
        sh = U(2 * (k - i))
        alive &= (x >> sh) == (y >> sh)
        n += alive
    return n


def issue(lists, captures):
    """the lookups of a batch: per query the forward lookup of every captured k-mer in its own mask's list and the reverse
    lookup of every distinct captured k-mer.  captures: [(kmers[M], loc_off[M + 1], locs)] per query.
    Returns a list of (query, list, direction, looked-up k-mer, source mask)"""
    out = []
    for q, (kmers, _off, _locs) in enumerate(captures):
        seen = set()
        for m, x in enumerate(kmers.tolist()):
            if x == 0:
                continue
            out.append((q, m, 0, x, m))
            if x not in seen:  # (ascending m: the first mask that captured it)
                seen.add(x)
                r = reverse_kmer(x, lists.k)
                out.append((q, lists.argmin_mask(r), 1, r, m))
    return out


FACTS = np.dtype([("query", "i8"), ("list", "i8"), ("dir", "i8"), ("partition", "i8"), ("outlier", "?"), ("nvalues", "i8"),
                  ("nloc", "i8"), ("lost", "?"), ("empty_partition", "?"), ("dropped", "?")])


def search(lists, captures, min_prefix, keep=None, lookups=None):
    """Returns (anchors, facts).
    anchors: per query {genome key: [n, 5] int64 rows (qbegin, tbegin, len, qrc, trc), sorted}: the raw multiset.
    facts: one FACTS record per lookup - list, partition (the anchor bases of the looked-up k-mer), outlier (the k-mer lacks
           the mask's prefix), nvalues (stored values in range and direction, whether the start rule loses them or not), nloc
           (query locations), lost (nvalues > 0 and the search starts behind the range), empty_partition (not an outlier, and
           the list holds no k-mer of the mask's prefix with these anchor bases), dropped (an outlier, and the list holds no
           outlier of this direction: the product does not even issue it).
    keep: a set of genome keys (the whitelist of (*Index).Search), or None."""
    K = lists.k
    low = U(4 ** (K - min_prefix) - 1) if min_prefix < K else U(0)
    lk = lookups if lookups is not None else issue(lists, captures)  # (they do not depend on min_prefix)
    by_list = {}
    for i, (_q, m, _d, _x, _src) in enumerate(lk):
        by_list.setdefault(m, []).append(i)
    facts = np.zeros(len(lk), dtype=FACTS)
    hit_lookup, hit_key, hit_val = [], [], []
    for m, ids in by_list.items():
        keys, vals = lists.keys[m], lists.vals[m]
        x = np.array([lk[i][3] for i in ids], dtype=U)
        d = np.array([lk[i][2] for i in ids], dtype=U)
        left, right = x & ~low, x | low
        in_range = (keys[None, :] >= left[:, None]) & (keys[None, :] <= right[:, None])
        take = in_range & ((vals[None, :] & U(1)) == d[:, None])
        nval = take.sum(axis=1)
        mask_pf = lists.prefix_of(lists.masks[m])
        outlier = lists.prefix_of(x) != mask_pf
        own = lists.prefix_of(keys) == mask_pf
        part = lists.anchor_of(x)
        own_anchors = set(lists.anchor_of(keys[own]).tolist())
        has_outlier = [bool((~own & ((vals & U(1)) == U(dd))).any()) for dd in (0, 1)]
        lost = np.zeros(len(ids), dtype=bool)
        if nval.any():
            index = lists.start_index(m)
            anchors_left = lists.anchor_of(left).tolist()
            for r in np.flatnonzero(nval):
                first = int(np.argmax(in_range[r]))  # the range's first position in the list
                lost[r] = index[anchors_left[r]] > first
        f = facts[ids]
        f["query"] = [lk[i][0] for i in ids]
        f["list"], f["dir"], f["partition"], f["outlier"], f["nvalues"], f["lost"] = m, d, part, outlier, nval, lost
        f["empty_partition"] = [not o and p not in own_anchors for o, p in zip(outlier.tolist(), part.tolist())]
        f["dropped"] = [o and not has_outlier[dd] for o, dd in zip(outlier.tolist(), d.tolist())]
        facts[ids] = f
        take[lost] = False
        r, c = np.nonzero(take)
        if len(r):
            hit_lookup.append(np.asarray(ids)[r])
            hit_key.append(keys[c])
            hit_val.append(vals[c])
    for i, (q, _m, _d, _x, src) in enumerate(lk):
        facts["nloc"][i] = captures[q][1][src + 1] - captures[q][1][src]
    assert not (facts["dropped"] & (facts["nvalues"] > 0)).any()
    nq = len(captures)
    anchors = [dict() for _ in range(nq)]
    if not hit_lookup:
        return anchors, facts
    hl, hk, hv = np.concatenate(hit_lookup), np.concatenate(hit_key), np.concatenate(hit_val)
    lq = np.array([t[0] for t in lk], dtype=np.int64)[hl]
    lx = np.array([t[3] for t in lk], dtype=U)[hl]
    lsrc = np.array([t[4] for t in lk], dtype=np.int64)[hl]
    ln = common_prefix(lx, hk, K)
    genome = (hv >> U(30)).astype(np.int64)
    pos_t = ((hv >> U(2)) & U((1 << 28) - 1)).astype(np.int64)
    rc_t = ((hv >> U(1)) & U(1)).astype(np.int64)
    rv = (hv & U(1)).astype(np.int64)
    if keep is not None:
        sel = np.isin(genome, np.fromiter(keep, dtype=np.int64, count=len(keep)))
        lq, lsrc, ln, genome, pos_t, rc_t, rv = (z[sel] for z in (lq, lsrc, ln, genome, pos_t, rc_t, rv))
    for q in range(nq):
        sel = np.flatnonzero(lq == q)
        if not len(sel):
            continue
        off, locs = captures[q][1], captures[q][2]
        nloc = off[lsrc[sel] + 1] - off[lsrc[sel]]
        rep = np.repeat(sel, nloc)  # one anchor per (value, query location)
        within = np.arange(len(rep)) - np.repeat(np.cumsum(nloc) - nloc, nloc)
        loc = locs[off[lsrc[rep]] + within]
        pos_q, rc_q = loc >> 1, loc & 1
        tail = K - ln[rep]
        # lib-index-search.go:1496-1524: a prefix match lies at the k-mer's start on its own strand, a suffix match (the
        # reversed k-mer) at its end
        fwd = rv[rep] == 0
        qb = np.where(fwd == (rc_q == 1), pos_q + tail, pos_q)
        tb = np.where(fwd == (rc_t[rep] == 1), pos_t[rep] + tail, pos_t[rep])
        tab = np.stack([genome[rep], qb, tb, ln[rep], rc_q, rc_t[rep]], axis=1)
        tab = tab[np.lexsort(tab.T[::-1])]
        cut = np.flatnonzero(tab[1:, 0] != tab[:-1, 0]) + 1
        for part in np.split(tab, cut):
            anchors[q][int(part[0, 0])] = part[:, 1:]
    return anchors, facts


def sorted_rows(rows):
    """[n, 5] rows in the model's order (lexicographic), for multiset comparison"""
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows
