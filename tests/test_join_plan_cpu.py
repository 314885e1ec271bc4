"""The record planner of lm_index_builder_add_index (lexicmap_amd/csrc/lm_join_plan.h) built for the host
(tests/join_plan_host.cpp): which records of a source are appended under which keys and chunk-list numbers, the key rewrite
table the decode kernel reads, the input-genome count, and every refusal - plus the new C-ABI declarations and wrappers."""
import ctypes as C
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "join_plan_host.cpp")
HDRS = [os.path.join(ROOT, "lexicmap_amd", "csrc", n) for n in ("lm_join_plan.h", "lm_build_plan.h")]
LIB = os.path.join(HERE, "libjoin_plan_host.so")
OK, EMPTY, UNKNOWN, REPEATED, HALF = 0, 1, 2, 3, 4


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", LIB, SRC])
    lib = C.CDLL(LIB)
    lib.jp_drop.restype = C.c_uint64
    return lib


def key(n, bs):
    return (n // bs) << 17 | n % bs


def plan(L, src, keep=None, next_record=0, batch_size=5000, next_list=0):
    """src: [(key, list or -1, list_n, list_idx)] in record order.  (0, dict) or (reason, text)"""
    n = len(src)
    u64, i32, i64 = C.c_uint64 * max(n, 1), C.c_int * max(n, 1), C.c_int64 * max(n, 1)
    a_key, a_list, a_n, a_idx = u64(*[s[0] for s in src]), i32(*[s[1] for s in src]), i32(*[s[2] for s in src]), i32(*[s[3] for s in src])
    kp = None if keep is None else (C.c_uint64 * max(len(keep), 1))(*keep)
    new_bg, k_src, k_num, k_key, k_list, k_n, k_idx = u64(), i64(), i64(), u64(), i32(), i32(), i32()
    nkept, nlists, drops, ninput = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    err = C.create_string_buffer(512)
    rc = L.jp_plan(a_key, a_list, a_n, a_idx, n, 0 if keep is None else 1, kp, 0 if keep is None else len(keep), C.c_int64(next_record),
                   batch_size, next_list, new_bg, C.byref(nkept), k_src, k_num, k_key, k_list, k_n, k_idx, C.byref(ninput), C.byref(nlists),
                   C.byref(drops), err, len(err))
    if rc != OK:
        return rc, err.value.decode()
    m = nkept.value
    return OK, dict(new_bg=list(new_bg[:n]), kept=[(k_src[i], k_num[i], k_key[i], k_list[i], k_n[i], k_idx[i]) for i in range(m)],
                    ninput=ninput.value, nlists=nlists.value, drops=bool(drops.value))


# a source of 7 records with batch size 3: records 1, 2 are split genome X (list 0), 4, 5, 6 split genome Y (list 1)
SRC7 = [(key(0, 3), -1, 0, 0), (key(1, 3), 0, 2, 0), (key(2, 3), 0, 2, 1), (key(3, 3), -1, 0, 0),
        (key(4, 3), 1, 3, 0), (key(5, 3), 1, 3, 1), (key(6, 3), 1, 3, 2)]


def test_whole_source_is_renumbered_across_a_batch_boundary(L):
    rc, p = plan(L, SRC7, None, next_record=3, batch_size=4, next_list=2)
    assert rc == OK
    want = [key(3 + i, 4) for i in range(7)]
    assert want[0] == 3 and want[1] == 1 << 17 and want[5] == (2 << 17)          # 3 closes batch 0, 4..7 are batch 1, 8 opens batch 2
    assert p["new_bg"] == want and not p["drops"]
    assert [(k[0], k[1], k[2]) for k in p["kept"]] == [(i, 3 + i, want[i]) for i in range(7)]
    # list ids moved up by the builder's next list id, shape and places kept
    assert [k[3:] for k in p["kept"]] == [(-1, 0, 0), (2, 2, 0), (2, 2, 1), (-1, 0, 0), (3, 3, 0), (3, 3, 1), (3, 3, 2)]
    assert p["nlists"] == 4
    assert p["ninput"] == 4                                                       # two plain genomes and two split ones


def test_scrambled_keep_list_gives_source_order(L):
    keep = [SRC7[i][0] for i in (6, 0, 4, 3, 5)]
    rc, p = plan(L, SRC7, keep, next_record=0, batch_size=2, next_list=5)
    assert rc == OK and p["drops"]
    assert [k[0] for k in p["kept"]] == [0, 3, 4, 5, 6]
    assert [k[1] for k in p["kept"]] == [0, 1, 2, 3, 4]
    assert [k[2] for k in p["kept"]] == [key(i, 2) for i in range(5)]
    drop = L.jp_drop()
    assert drop == 2 ** 64 - 1
    assert p["new_bg"] == [key(0, 2), drop, drop, key(1, 2), key(2, 2), key(3, 2), key(4, 2)]
    # the one kept list is the builder's next one, whatever its number in the source was
    assert [k[3:] for k in p["kept"]] == [(-1, 0, 0), (-1, 0, 0), (5, 3, 0), (5, 3, 1), (5, 3, 2)]
    assert p["nlists"] == 6 and p["ninput"] == 3


def test_source_list_numbers_need_not_be_dense_or_ordered(L):
    src = [(10, 7, 2, 0), (11, 7, 2, 1), (12, 3, 2, 0), (13, 3, 2, 1), (14, -1, 0, 0)]
    rc, p = plan(L, src, None, next_record=10, batch_size=5000, next_list=0)
    assert rc == OK
    assert [k[3] for k in p["kept"]] == [0, 0, 1, 1, -1] and p["nlists"] == 2 and p["ninput"] == 3
    assert p["new_bg"] == [10, 11, 12, 13, 14]


def test_single_record_kept(L):
    rc, p = plan(L, SRC7, [SRC7[3][0]], next_record=0, batch_size=5000)
    assert rc == OK and p["drops"] and p["ninput"] == 1 and p["nlists"] == 0
    assert p["kept"] == [(3, 0, 0, -1, 0, 0)]
    assert p["new_bg"].count(L.jp_drop()) == 6


def test_refusals(L):
    rc, txt = plan(L, SRC7, [SRC7[0][0], 99 << 17 | 5])
    assert rc == UNKNOWN and "no record of the source" in txt and "batch 99, index 5" in txt
    rc, txt = plan(L, SRC7, [SRC7[0][0], SRC7[3][0], SRC7[0][0]])
    assert rc == REPEATED and "twice" in txt
    rc, txt = plan(L, SRC7, [SRC7[0][0], SRC7[4][0], SRC7[6][0]])
    assert rc == HALF and "2 of the 3 records of a split genome" in txt
    rc, txt = plan(L, SRC7, [SRC7[2][0]])
    assert rc == HALF and "1 of the 2" in txt
    rc, txt = plan(L, SRC7, [])
    assert rc == EMPTY and "empty" in txt
    rc, txt = plan(L, [], None)
    assert rc == EMPTY
    # a split genome whose other records are not in the source's table at all cannot be taken either
    rc, txt = plan(L, [(0, 0, 2, 0), (1, -1, 0, 0)], None)
    assert rc == HALF


def test_declarations_and_wrappers(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "lexicmap_hip.h")).read()
    assert re.search(r"lm_status lm_index_builder_add_index\(lm_index_builder \*b, lm_index \*src, const uint64_t \*keep, size_t nkeep\);", hdr)
    assert re.search(r"lm_status lm_index_builder_like\(const lm_index \*model, const lm_build_opt \*bo, const lm_residency \*res, "
                     r"lm_index_builder \*\*out\);", hdr)
    # still C99
    c = str(tmp_path / "hdr_check.c")
    open(c, "w").write('#include "%s"\nint main(void) { return 0; }\n' % os.path.join(ROOT, "include", "lexicmap_hip.h"))
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", c])
    from lexicmap_amd import api
    for cls, names in ((api.IndexBuilder, ("add_index", "try_add_index", "like")), (api.Index, ("join", "subset"))):
        for n in names:
            assert callable(getattr(cls, n))
