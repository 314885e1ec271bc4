"""-a/--all through the host shard merge: lm_merge_sharded_ex(..., LM_ROW_ALL) copies the cigar / qseq / sseq / align strings of
the input rows (live in this process) into the result, each following its row into the merged order; with flags 0 and through
lm_merge_sharded the string columns stay NULL.  Host-only: no GPU needed."""
import ctypes as C

import numpy as np
import pytest

from lexicmap_amd import merge
from lexicmap_amd.api import Hsp, LM_ROW_ALL, lib, row_strings

# rows per shard; shard 1 has none
SHARD_ROWS = (260, 0, 310)


def _strings(rng, uid):
    """the four string columns of row `uid`: NULL, empty, short and (one row) a 100-kb string"""
    if uid % 11 == 3:
        return (None, None, None, None)
    out = []
    for k in range(4):
        r = (uid * 7 + k) % 9
        if r == 0:
            out.append(None)
        elif r == 1:
            out.append(b"")
        else:
            n = int(rng.integers(1, 90))
            out.append(bytes(rng.choice(list(b"ACGTMID|. "), n).tolist()) + b"%d.%d" % (uid, k))
    if uid == 17:
        out[1] = b"A" * 100_000 + b"Z"
    return tuple(out)


def _shards():
    """per-shard rows grouped by query, a genome's rows together and in ONE shard; ties of the best similarity across shards and
    within a shard; matched_bases = a unique row id (which input row an output row came from)"""
    rng = np.random.default_rng(11)
    shards, strs, keep = [], {}, []
    uid = 0
    for r, n in enumerate(SHARD_ROWS):
        arr = np.zeros(n, dtype=merge.ROW_DTYPE)
        qs = np.sort(rng.integers(0, 12, n))
        gs = rng.integers(0, 8, n) * len(SHARD_ROWS) + r
        o = np.lexsort((gs, qs))
        arr["query"], arr["batch_genome"] = qs[o], gs[o]
        arr["bitscore"] = rng.choice([100, 200, 300], n)   # few distinct values: ties of the best similarity
        arr["pident"] = rng.choice([90.0, 100.0], n)
        arr["qcov_hsp"] = rng.random(n)
        for i in range(n):
            arr["matched_bases"][i] = uid
            s = _strings(rng, uid)
            strs[uid] = s
            for f, x in zip(("cigar", "qseq", "sseq", "align"), s):
                if x is not None:
                    b = C.create_string_buffer(x)
                    keep.append(b)
                    arr[f][i] = C.addressof(b)
            uid += 1
        shards.append(arr)
    return shards, strs, keep


def _cols(a):
    return [(f, np.ascontiguousarray(a[f]).tobytes()) for f in merge.ROW_DTYPE.names if f not in merge.PTR_FIELDS]


def test_strings_follow_their_rows_through_the_host_merge():
    shards, strs, keep = _shards()
    want = merge.merge_sharded(shards)                     # the numpy statement of the order (pointer columns cleared)
    got = merge.merge_sharded_c(shards, strings=True)      # a view: its pointer columns live while it is alive
    assert len(got) == sum(SHARD_ROWS) == len(want)
    assert _cols(got) == _cols(want)
    assert (got["genome_id"] == 0).all() and (got["seq_id"] == 0).all()   # no index: no names
    seen = set()
    for i in range(len(got)):
        uid = int(got["matched_bases"][i])
        exp = tuple(None if x is None else x.decode() for x in strs[uid])
        assert row_strings(got, i) == exp, i
        seen.add(uid)
    assert len(seen) == len(got)
    assert any(s == (None, None, None, None) for s in strs.values())
    assert any(x == b"" for s in strs.values() for x in s)
    assert max(len(got_s or "") for i in range(len(got)) for got_s in row_strings(got, i)) == 100_001
    # the result owns its copies: the input buffers may go
    del keep
    uid = int(got["matched_bases"][0])
    assert row_strings(got, 0) == tuple(None if x is None else x.decode() for x in strs[uid])


def test_without_the_flag_the_string_columns_stay_null():
    shards, strs, keep = _shards()
    plain = merge.merge_sharded_c(shards)                  # lm_merge_sharded_ex with flags 0
    L = lib()
    arrs = [np.ascontiguousarray(p, dtype=merge.ROW_DTYPE) for p in shards]
    ptrs = (C.POINTER(Hsp) * 3)(*[a.ctypes.data_as(C.POINTER(Hsp)) for a in arrs])
    cnts = (C.c_size_t * 3)(*[len(a) for a in arrs])
    res = C.c_void_p()
    assert L.lm_merge_sharded(None, ptrs, cnts, 3, C.byref(res)) == 0
    rows_p = C.POINTER(Hsp)()
    k = L.lm_result_rows(res, C.byref(rows_p))
    old = np.zeros(k, dtype=merge.ROW_DTYPE)
    C.memmove(old.ctypes.data, rows_p, k * C.sizeof(Hsp))
    L.lm_result_free(res)
    withs = merge.merge_sharded_c(shards, strings=True)
    for a in (plain, old):
        assert len(a) == sum(SHARD_ROWS)
        assert _cols(a) == _cols(withs)
        for f in merge.PTR_FIELDS:
            assert (a[f] == 0).all(), f
    # a flag other than LM_ROW_ALL is refused
    res = C.c_void_p()
    assert L.lm_merge_sharded_ex(None, ptrs, cnts, 3, 4, C.byref(res)) == 7   # LM_ERR_ARG
    assert L.lm_merge_sharded_ex(None, ptrs, cnts, 3, LM_ROW_ALL, C.byref(res)) == 0
    L.lm_result_free(res)


@pytest.mark.parametrize("rows", [0, 1])
def test_empty_and_single_row_merges_with_strings(rows):
    arr = np.zeros(rows, dtype=merge.ROW_DTYPE)
    keep = []
    if rows:
        b = C.create_string_buffer(b"10M")
        keep.append(b)
        arr["cigar"][0] = C.addressof(b)
    got = merge.merge_sharded_c([arr, arr[:0]], strings=True)
    assert len(got) == rows
    if rows:
        assert row_strings(got, 0) == ("10M", None, None, None)
