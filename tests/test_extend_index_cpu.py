"""lm_index_builder_extend without a GPU: the declaration (exported by the cross-compiled library, header still C99), the
continued record numbering (key and shard rule of lm_build_plan.h at record numbers behind a base), and the seed-number ->
list / partition walk of k_sp_dump_range (lm_seed_walk.h, built for the host) against a plain loop over the tables."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "lexicmap_amd", "csrc")


def _host_lib(name, src, hdr):
    lib = os.path.join(HERE, "lib%s.so" % name)
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", lib, src])
    return C.CDLL(lib)


def test_extend_is_declared_exported_and_the_header_is_c99():
    import lexicmap_amd as la
    la.build_library()
    hdr = os.path.join(ROOT, "include", "lexicmap_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert re.search(r"lm_status\s+lm_index_builder_extend\s*\(\s*lm_index\s*\*\s*\w+\s*,\s*const\s+lm_build_opt\s*\*\s*\w+\s*,"
                     r"\s*const\s+lm_residency\s*\*\s*\w+\s*,\s*lm_index_builder\s*\*\*\s*\w+\s*\)\s*;", txt)
    out = subprocess.check_output(["nm", "-D", "--defined-only", la.LIB_PATH]).decode()
    assert "lm_index_builder_extend" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert hasattr(la.Index, "extend") and hasattr(la.IndexBuilder, "extending")


def test_numbering_continues_behind_a_base():
    L = _host_lib("build_plan_host", os.path.join(HERE, "build_plan_host.cpp"), os.path.join(CSRC, "lm_build_plan.h"))
    L.bp_key.argtypes = [C.c_int64, C.c_int]
    L.bp_key.restype = C.c_uint64
    L.bp_keeps.argtypes = [C.c_int64, C.c_int, C.c_int]
    # a base of 5 records in batches of 4: the added records 5, 6, 7 finish batch 1 and record 8 opens batch 2
    assert [L.bp_key(n, 4) for n in range(5, 9)] == [(1 << 17) | 1, (1 << 17) | 2, (1 << 17) | 3, 2 << 17]
    # the key of a record does not depend on where a build began: base of 7 999 records, default batches
    assert [L.bp_key(n, 5000) for n in (7999, 9999, 10000)] == [(1 << 17) | 2999, (1 << 17) | 4999, 2 << 17]
    # the shard of a genome is that of its FIRST record number, counted over all shards of the base
    assert [bool(L.bp_keeps(n, 2, 1)) for n in (5, 6, 7, 8)] == [True, False, True, False]
    assert all(L.bp_keeps(n, 1, 0) for n in (5, 8))


@pytest.fixture(scope="module")
def W():
    lib = _host_lib("seed_walk_host", os.path.join(HERE, "seed_walk_host.cpp"), os.path.join(CSRC, "lm_seed_walk.h"))
    i64p = C.POINTER(C.c_int64)
    lib.sw_walk.argtypes = [i64p, C.POINTER(C.c_uint32), C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int,
                            C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.sw_lists_of_piece.argtypes = [i64p, C.c_int64, C.c_int64, C.c_int64, i64p, i64p]
    return lib


def _image(rng, n, P, sizes):
    """off[n + 1], tab[n][P + 1] and the plain answer (list, partition) of every seed"""
    off, tab, truth = [0], [], []
    for l in range(n):
        cnt = [rng.choice(sizes) for _ in range(P)]
        row = [0]
        for p, c in enumerate(cnt):
            truth += [(l, p)] * c
            row.append(row[-1] + c)
        tab += row
        off.append(off[-1] + row[-1])
    return off, tab, truth


@pytest.mark.parametrize("sizes,tile", [((0, 0, 0, 1), 64), ((0, 1, 2, 7), 256), ((0, 0, 40, 300), 256), ((0,) * 30 + (5000,), 256)])
def test_list_and_partition_walk_equals_a_plain_loop(W, sizes, tile):
    """lists and partitions that are mostly empty, shorter than a tile, longer than a tile; pieces that begin and end inside a
    list, inside a partition, on a boundary; a piece of one seed"""
    rng = random.Random(7)
    n, P = 12, 16
    off, tab, truth = _image(rng, n, P, sizes)
    N = off[-1]
    assert N == len(truth) and N > 0
    offa = (C.c_int64 * len(off))(*off)
    taba = (C.c_uint32 * len(tab))(*tab)
    cuts = sorted({0, N, N // 3, N // 2, max(0, N - 1)} | {rng.randrange(N + 1) for _ in range(6)} | set(o for o in off))
    pieces = [(a, b) for a in cuts for b in cuts if a < b][:60] + [(N // 2, N // 2 + 1)]
    for s0, s1 in pieces:
        ol, op = (C.c_int32 * (s1 - s0))(), (C.c_int32 * (s1 - s0))()
        W.sw_walk(offa, taba, n, P, s0, s1, tile, ol, op)
        assert list(zip(ol, op)) == truth[s0:s1], (s0, s1)
        l0, l1 = C.c_int64(), C.c_int64()
        W.sw_lists_of_piece(offa, n, s0, s1, C.byref(l0), C.byref(l1))
        assert (l0.value, l1.value) == (truth[s0][0], truth[s1 - 1][0] + 1)
