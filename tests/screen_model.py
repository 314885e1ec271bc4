"""Genome screening (GSearchScreen, lib-index-search-genome.go:114-543) restated over the CPU oracle only: the yardstick of
lm_index_screen_genomes.  Masking is lmo_lh_mask per window, the drop rule lmo_low_complexity, the lookup lmo_kv_load /
lmo_kv_search2(p, 1, 0) over the seeds/chunk_*.bin files of an index the oracle's writer made; accumulation, chunk merge,
order and cut are plain Python.  Nothing here calls lexicmap_amd.

Where the reference is not deterministic the model takes the rule the library documents: a split genome's details are those
of its hit record with the lowest key; rows of equal score are ordered by ascending lowest key."""
import ctypes as C
import glob
import os

import oracle as O


class KvSr(C.Structure):
    _fields_ = [("iquery", C.c_int), ("iquery2", C.c_int), ("len", C.c_uint8), ("is_suffix", C.c_uint8),
                ("val_off", C.c_int64), ("nvals", C.c_int)]


class KvResults(C.Structure):
    _fields_ = [("sr", C.POINTER(KvSr)), ("n", C.c_int), ("cap", C.c_int), ("vals", C.POINTER(C.c_uint64)),
                ("nv", C.c_int64), ("capv", C.c_int64)]


class KvMem(C.Structure):
    _fields_ = [("k", C.c_int), ("chunk_index", C.c_int), ("chunk_size", C.c_int), ("mask_prefix", C.c_int),
                ("anchor_prefix", C.c_int), ("use7", C.c_int)]   # (the head of lmo_kv_mem: what the model reads)


_bound = False


def _lib():
    global _bound
    L = O.lib()
    if not _bound:
        L.lmo_kv_load.restype = C.POINTER(KvMem)
        L.lmo_kv_load.argtypes = [C.c_char_p]
        L.lmo_kv_free.argtypes = [C.POINTER(KvMem)]
        L.lmo_kv_search2.argtypes = [C.POINTER(KvMem), C.POINTER(C.c_uint64), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int,
                                     C.POINTER(KvResults)]
        L.lmo_kv_results_free.argtypes = [C.POINTER(KvResults)]
        _bound = True
    return L


_TAB = bytearray(b"A" * 256)
for _src, _dst in ((b"Aa", b"A"), (b"CcBbSsYy", b"C"), (b"GgKk", b"G"), (b"TtUu", b"T")):
    for _c in _src:
        _TAB[_c] = _dst[0]
_TAB = bytes(_TAB)   # baseConvert, search-genome-util.go:227-244 (= genome_build_fixture.concatenation's table)


def query_layout(contigs, k, n_runs_skipped=False):
    """(bigSeq, skip regions) of a query genome, search-genome-util.go:155-182: contigs through the base table, joined by k
    skipped bases; the regions are exactly those spacers.  n_runs_skipped: ALSO the runs of >= 5 N of the raw contigs, as the
    index builder would skip them (lib-gaps.go:38-60) - not what screening does; there for tests that show the difference."""
    seq, regions = bytearray(), []
    for i, (_, s) in enumerate(contigs):
        if i > 0:
            regions.append((len(seq), len(seq) + k - 1))
            seq += b"A" * k
        base = len(seq)
        s = bytes(s)
        if n_runs_skipped:
            j = 0
            while j < len(s):
                if s[j] in b"Nn":
                    e = j
                    while e < len(s) and s[e] in b"Nn":
                        e += 1
                    if e - j >= 5:
                        regions.append((base + j, base + e - 1))
                    j = e
                else:
                    j += 1
        seq += s.translate(_TAB)
    return bytes(seq), sorted(regions)


def windows_of(n, windows):
    """lib-index-search-genome.go:150-173"""
    step = n // (windows + 1)
    window = n if windows == 1 else step * 2
    return [(i * step, n if i == windows - 1 else i * step + window) for i in range(windows)]


def chunk_lists(records):
    """key lists of the split genomes of genome_build_fixture.records(...) (consecutive records of one genome id; keys of a
    set within one genome batch are the record numbers)"""
    out, i = [], 0
    while i < len(records):
        j = i
        while j + 1 < len(records) and records[j + 1][0] == records[i][0]:
            j += 1
        if j > i:
            out.append(list(range(i, j + 1)))
        i = j + 1
    return out


def merge_order_cut(per_record, lists, top_n):
    """per_record: {key: dict(score=..., [details])} of one query -> rows (lib-index-search-genome.go:423-509)"""
    list_of = {key: i for i, ks in enumerate(lists) for key in ks}
    rows, row_of_list = [], {}
    for key in sorted(per_record):
        r = per_record[key]
        li = list_of.get(key)
        if li is not None and li in row_of_list:
            row = row_of_list[li]
            row["score"] += r["score"]
            row["keys"].append(key)
            continue
        row = dict(r, batch_genome=key, keys=[key])
        if li is not None:
            row_of_list[li] = row
        rows.append(row)
    rows.sort(key=lambda r: (-r["score"], r["batch_genome"]))
    return rows[:top_n] if top_n > 0 else rows


class Model:
    def __init__(self, index_dir, k, masks, lists=(), names=None):
        """index_dir: an index written by oracle.build_index; masks: its mask set; lists: key lists of split genomes;
        names: {key: genome id}"""
        L = _lib()
        self.k, self.M = k, len(masks)
        self.lists = [list(x) for x in lists]
        self.names = names or {}
        arr = (C.c_uint64 * self.M)(*masks)
        self.lh = L.lmo_lh_new(k, arr, self.M)
        self.chunks, self._cache = [], {}
        for f in sorted(glob.glob(os.path.join(index_dir, "seeds", "chunk_*.bin"))):
            m = L.lmo_kv_load(f.encode())
            assert m, f
            self.chunks.append(m)
        assert self.chunks

    def close(self):
        L = _lib()
        for m in self.chunks:
            L.lmo_kv_free(m)
        self.chunks = []
        if self.lh:
            L.lmo_lh_free(self.lh)
            self.lh = None

    def min_prefix_range(self):
        m = self.chunks[0].contents
        return m.mask_prefix + m.anchor_prefix, self.k

    def kmers(self, contigs, windows=1, n_runs_skipped=False):
        """per mask the sorted, de-duplicated captures of all windows (:167-207)"""
        L = _lib()
        seq, regions = query_layout(contigs, self.k, n_runs_skipped)
        per_mask = [set() for _ in range(self.M)]
        if len(seq) < self.k:
            return per_mask
        flat = [x for r in regions for x in r]
        skip = (C.c_int * max(len(flat), 1))(*flat)
        out = (C.c_uint64 * self.M)()
        for s, e in windows_of(len(seq), windows):
            if e - s < self.k:
                continue
            loc_off, locs = C.POINTER(C.c_int)(), C.POINTER(C.c_int)()
            # (:180: the slice is masked with the UNSHIFTED regions of the whole sequence)
            L.lmo_lh_mask(self.lh, seq[s:e], e - s, skip, len(regions), 1, out, C.byref(loc_off), C.byref(locs))
            L.free(loc_off)
            L.free(locs)
            for m in range(self.M):
                x = out[m]
                if x != 0 and not L.lmo_low_complexity(x, self.k):
                    per_mask[m].add(x)
        return per_mask

    def per_record(self, contigs, min_prefix=21, windows=1, keep=None, n_runs_skipped=False):
        """{record key: dict(score, hits[M], longest[M], values[M])} - lib-index-search-genome.go:255-341.  Computed once
        per distinct input and shared (callers do not change it)."""
        ck = (tuple((c, bytes(s)) for c, s in contigs), min_prefix, windows, None if keep is None else frozenset(keep), n_runs_skipped)
        if ck not in self._cache:
            self._cache[ck] = self._per_record(contigs, min_prefix, windows, keep, n_runs_skipped)
        return self._cache[ck]

    def _per_record(self, contigs, min_prefix, windows, keep, n_runs_skipped):
        L = _lib()
        per_mask = self.kmers(contigs, windows, n_runs_skipped)
        acc = {}
        for mem in self.chunks:
            c = mem.contents
            off, flat = [0], []
            for m in range(c.chunk_index, c.chunk_index + c.chunk_size):
                flat += sorted(per_mask[m])
                off.append(len(flat))
            res = KvResults()
            rc = L.lmo_kv_search2(mem, (C.c_uint64 * max(len(flat), 1))(*flat), (C.c_int * len(off))(*off), min_prefix, 1, 0,
                                  C.byref(res))
            assert rc == 0, rc
            for i in range(res.n):
                sr = res.sr[i]
                for j in range(sr.nvals):
                    key = res.vals[sr.val_off + j] >> 30
                    if keep is not None and key not in keep:
                        continue
                    r = acc.get(key)
                    if r is None:
                        r = acc[key] = dict(score=0, hits=[0] * self.M, longest=[0] * self.M, values=[0] * self.M)
                    r["values"][sr.iquery] += 1   # (unsaturated: for tests that want to see Hits saturate)
                    if r["hits"][sr.iquery] < 255:
                        r["hits"][sr.iquery] += 1
                    if r["longest"][sr.iquery] < sr.len:
                        r["longest"][sr.iquery] = sr.len
                    r["score"] += sr.len
            L.lmo_kv_results_free(C.byref(res))
        return acc

    def screen_one(self, contigs, min_prefix=21, windows=1, top_n=10, details=False, keep=None, n_runs_skipped=False):
        acc = self.per_record(contigs, min_prefix, windows, keep, n_runs_skipped)
        recs = {}
        for key, r in acc.items():
            d = dict(score=r["score"], score2=0, hit_masks=0, hit_kmers=0, prefixes=[], genome_id=self.names.get(key))
            if details:   # :412-419, search-genome.go:554-591
                d["hit_masks"] = sum(1 for h in r["hits"] if h > 0)
                d["hit_kmers"] = sum(r["hits"])
                d["score2"] = sum(r["longest"])
                d["prefixes"] = sorted((l for h, l in zip(r["hits"], r["longest"]) if h > 0), reverse=True)
            recs[key] = d
        return merge_order_cut(recs, self.lists, top_n)

    def screen(self, genomes, **kw):
        return [self.screen_one(contigs, **kw) for _, contigs in genomes]


def format_rows(rows, query_ids, min_prefix, masks, extra=False):
    """search-genome.go:577-590 with Python's own %-formatting"""
    out = []
    for qid, qrows in zip(query_ids, rows):
        for r in qrows:
            gid = r["genome_id"]
            gid = gid.decode() if isinstance(gid, bytes) else gid
            line = "%s\t%s\t%d\t%.4f\t%d\t%d\t%.2f" % (qid, gid, min_prefix, r["hit_masks"] / masks, r["hit_masks"], r["score2"],
                                                       r["score2"] / r["hit_masks"])
            if extra:
                line += "\t" + ",".join(str(p) for p in r["prefixes"])
            out.append(line)
    return out
