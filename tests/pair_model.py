"""`lexicmap genome pair -s 0` (lexicmap/cmd/pair.go) restated in plain Python over the CPU oracle only: the yardstick of
lm_index_genome_pairs.  Each mask's interleaved (k-mer, value) list comes from lmo_kv_load of an index the oracle's writer
made; the forward seeds (value & 1 == 0) are grouped by their top min_prefix bases and every group is paired by a
brute-force double loop.  Nothing here calls lexicmap_amd."""
import ctypes as C
import glob
import os

import oracle as O


class KvMem(C.Structure):
    _fields_ = [("k", C.c_int), ("chunk_index", C.c_int), ("chunk_size", C.c_int), ("mask_prefix", C.c_int),
                ("anchor_prefix", C.c_int), ("use7", C.c_int), ("kv", C.POINTER(C.POINTER(C.c_uint64))),
                ("kvlen", C.POINTER(C.c_int64))]   # (the head of lmo_kv_mem)


def select_masks(masks, k, nmasks):
    """pair.go:162-184 -> the selected mask numbers; ValueError for a refused nmasks"""
    if nmasks == 0:
        return list(range(len(masks)))
    q, x = 0, nmasks
    while x > 1 and x % 4 == 0:
        x //= 4
        q += 1
    if nmasks < 64 or x != 1 or nmasks > len(masks):
        raise ValueError("masks = %d" % nmasks)
    seen, out = set(), []
    for i, m in enumerate(masks):
        p = m >> (2 * (k - q))
        if p not in seen:
            seen.add(p)
            out.append(i)
    return out


def required(frac, total):
    return int(frac * float(total))   # pair.go:236


def lcp(a, b, k):
    return k if a == b else (64 - (a ^ b).bit_length()) // 2 + k - 32   # pair.go:903, :943


def order(rows):
    """pair.go:995-1004; rows: (key1, key2, n_masks, sum_prefix)"""
    return sorted(rows, key=lambda r: (-r[2], -r[3], r[0], r[1]))


class Model:
    def __init__(self, index_dir, k, masks):
        """index_dir: an index written by oracle.build_index with the mask set `masks`"""
        L = O.lib()
        L.lmo_kv_load.restype = C.POINTER(KvMem)
        L.lmo_kv_load.argtypes = [C.c_char_p]
        L.lmo_kv_free.argtypes = [C.POINTER(KvMem)]
        self.k, self.masks = k, list(masks)
        self.fwd = [None] * len(masks)   # per mask the forward seeds (k-mer, record key), in list order
        self.mask_prefix = self.anchor_prefix = None
        for f in sorted(glob.glob(os.path.join(index_dir, "seeds", "chunk_*.bin"))):
            mem = L.lmo_kv_load(f.encode())
            assert mem, f
            c = mem.contents
            self.mask_prefix, self.anchor_prefix = c.mask_prefix, c.anchor_prefix
            for i in range(c.chunk_size):
                n = c.kvlen[i]
                kv = c.kv[i][:n] if n else []
                self.fwd[c.chunk_index + i] = [(kv[j], kv[j + 1] >> 30) for j in range(0, n, 2) if kv[j + 1] & 1 == 0]
            L.lmo_kv_free(mem)
        assert all(x is not None for x in self.fwd)
        self._cache = {}

    def min_prefix_range(self):
        return self.mask_prefix + self.anchor_prefix, self.k

    def groups(self, m, min_prefix, keys=None):
        """the groups of mask m: lists of (k-mer, record), by kmer >> 2 (k - min_prefix), in ascending group order"""
        g = {}
        for x, r in self.fwd[m]:
            if keys is None or r in keys:
                g.setdefault(x >> (2 * (self.k - min_prefix)), []).append((x, r))
        return [g[p] for p in sorted(g)]

    def run(self, min_prefix=21, masks=1024, keys=None):
        """-> dict(total, pairs = {(key1, key2): [n_masks, sum_prefix]}, tuples, same_record, largest_group): every pair that
        matched under some selected mask; computed once per distinct input and shared (callers do not change it)"""
        ck = (min_prefix, masks, None if keys is None else frozenset(keys))
        if ck in self._cache:
            return self._cache[ck]
        keyset = None if keys is None else set(keys)
        sel = select_masks(self.masks, self.k, masks)
        pairs, tuples, same, largest = {}, 0, 0, 0
        for m in sel:
            best = {}
            for grp in self.groups(m, min_prefix, keyset):
                largest = max(largest, len(grp))
                for j in range(len(grp)):
                    xj, rj = grp[j]
                    for i in range(j):
                        xi, ri = grp[i]
                        tuples += 1
                        if ri == rj:
                            same += 1
                            continue
                        key = (ri, rj) if ri < rj else (rj, ri)
                        l = lcp(xi, xj, self.k)
                        if best.get(key, 0) < l:
                            best[key] = l
            for key, l in best.items():
                e = pairs.setdefault(key, [0, 0])
                e[0] += 1
                e[1] += l
        out = dict(total=len(sel), pairs=pairs, tuples=tuples, same_record=same, largest_group=largest)
        self._cache[ck] = out
        return out

    def rows(self, min_prefix=21, masks=1024, min_mask_fraction=0.25, keys=None):
        """the rows in output order: (key1, key2, n_masks, sum_prefix)"""
        r = self.run(min_prefix, masks, keys)
        req = required(min_mask_fraction, r["total"])
        return order([(a, b, n, s) for (a, b), (n, s) in r["pairs"].items() if n >= req])

    def structure(self, min_prefix):
        """(outlier entries, groups made only of outliers that hold two records, mixed groups) over all masks: an outlier is a
        forward seed whose k-mer lacks its mask's prefix"""
        p = self.mask_prefix
        n_out = only = mixed = 0
        for m in range(len(self.masks)):
            mp = self.masks[m] >> (2 * (self.k - p))
            for grp in self.groups(m, min_prefix):
                o = [(x >> (2 * (self.k - p))) != mp for x, _ in grp]
                n_out += sum(o)
                if all(o) and len({r for _, r in grp}) > 1:
                    only += 1
                if any(o) and not all(o):
                    mixed += 1
        return n_out, only, mixed


def format_rows(rows, names, min_prefix, total):
    """pair.go:730 with Python's own %-formatting; names: {key: genome id}"""
    return ["%s\t%s\t%d\t%.4f\t%d\t%d\t%.2f" % (names[a], names[b], min_prefix, n / total, n, s, s / n) for a, b, n, s in rows]


HEADER = "genome1\tgenome2\tminPrefix\tfracMasks\tnMasks\tsumPrefix\tavgPrefix"   # pair.go:721
