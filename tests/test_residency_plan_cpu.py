"""The genome placement planner (lexicmap_amd/csrc/lm_residency.h) built for the host (tests/residency_host.cpp): which
genomes stay in the device store and which go to pinned host segments for a byte budget, and the byte range
k_stage_genome_bits copies for a chain window of a host-resident genome."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "residency_host.cpp")
HDR = os.path.join(os.path.dirname(HERE), "lexicmap_amd", "csrc", "lm_residency.h")
LIB = os.path.join(HERE, "libresidency_host.so")
AUTO, DEVICE, HOST = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
    lib = C.CDLL(LIB)
    lib.rh_plan.argtypes = [C.POINTER(C.c_int64), C.c_int64, C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_int32),
                            C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64)]
    for f in ("rh_device_slot", "rh_host_slot"):
        getattr(lib, f).argtypes = [C.c_int64]
        getattr(lib, f).restype = C.c_int64
    lib.rh_stage_range.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int64)]
    return lib


def plan(L, sizes, mode, budget, seg_cap=1 << 32):
    n = len(sizes)
    b = (C.c_int64 * max(n, 1))(*sizes)
    seg = (C.c_int32 * max(n, 1))()
    off = (C.c_int64 * max(n, 1))()
    segs = (C.c_int64 * (n + 1))()
    tot = (C.c_int64 * 4)()
    ns = L.rh_plan(b, n, mode, budget, seg_cap, seg, off, segs, n + 1, tot)
    return dict(seg=list(seg)[:n], off=list(off)[:n], segs=list(segs)[:ns], ndev=tot[0], nhost=tot[1], bdev=tot[2], bhost=tot[3])


def dslot(n):   # the device store's layout: 8 .. 15 bytes of padding, the next genome at a multiple of 8
    return (n + 15) & ~7


def hslot(n):   # a pinned segment's: genomes at multiples of 16, 16 .. 31 bytes of padding
    return ((n + 15) & ~15) + 16


def test_slot_sizes(L):
    for n in (0, 1, 7, 8, 9, 15, 16, 17, 100_001, 1 << 26):
        assert L.rh_device_slot(n) == dslot(n) and 8 <= dslot(n) - n <= 15
        assert L.rh_host_slot(n) == hslot(n) and 16 <= hslot(n) - n <= 31 and hslot(n) % 16 == 0


def test_host_request_and_zero_budget_put_everything_on_the_host(L):
    sizes = [100_003, 5, 250_000, 99_999]
    for mode, budget in ((HOST, 0), (HOST, 1 << 40), (AUTO, 0)):
        p = plan(L, sizes, mode, budget)
        assert p["ndev"] == 0 and p["nhost"] == 4 and p["bdev"] == 0
        assert all(s >= 0 for s in p["seg"])
        assert p["bhost"] == sum(hslot(n) for n in sizes) == sum(p["segs"])


def test_budget_at_or_above_the_total_keeps_everything_on_the_device(L):
    sizes = [100_003, 5, 250_000, 99_999]
    total = sum(dslot(n) for n in sizes)
    for mode, budget in ((AUTO, total), (AUTO, total + 1), (AUTO, 1 << 40), (DEVICE, 0), (DEVICE, 17)):
        p = plan(L, sizes, mode, budget)
        assert p["ndev"] == 4 and p["nhost"] == 0 and p["segs"] == [] and p["bhost"] == 0
        assert p["bdev"] == total
        # today's offsets: the running sum of the padded sizes
        acc = 0
        for n, s, o in zip(sizes, p["seg"], p["off"]):
            assert s == -1 and o == acc
            acc += dslot(n)
    p = plan(L, sizes, AUTO, total - 1)   # one byte short: the last genome goes
    assert p["ndev"] == 3 and p["nhost"] == 1 and p["seg"] == [-1, -1, -1, 0]


def test_split_is_a_prefix_deterministic_and_never_cuts_a_genome(L):
    rng = random.Random(11)
    for trial in range(200):
        n = rng.randint(1, 40)
        sizes = [rng.choice([rng.randint(0, 64), rng.randint(1000, 400_000)]) for _ in range(n)]
        total = sum(dslot(x) for x in sizes)
        budget = rng.randint(0, total + 100)
        cap = rng.choice([1 << 32, 500_000, 64, 1 << 20])
        p = plan(L, sizes, AUTO, budget, cap)
        assert p == plan(L, sizes, AUTO, budget, cap)   # nothing but sizes, budget and cap decide
        nd = p["ndev"]
        assert p["seg"][:nd] == [-1] * nd and all(s >= 0 for s in p["seg"][nd:])   # a prefix stays, the rest goes
        assert p["bdev"] == sum(dslot(x) for x in sizes[:nd]) <= budget
        if nd < n:   # the first host genome is the first that did not fit
            assert p["bdev"] + dslot(sizes[nd]) > budget
        assert p["bhost"] == sum(hslot(x) for x in sizes[nd:]) == sum(p["segs"])   # padding accounted
        # whole genomes inside one segment each, in order, back to back, 16-byte aligned, never past the cap
        fill = {}
        for x, s, o in zip(sizes[nd:], p["seg"][nd:], p["off"][nd:]):
            assert o % 16 == 0 and o == fill.get(s, 0)
            fill[s] = o + hslot(x)
            assert fill[s] <= p["segs"][s]
        assert sorted(fill) == list(range(len(p["segs"])))
        for s, b in enumerate(p["segs"]):
            assert fill[s] == b
            alone = sum(1 for q in p["seg"][nd:] if q == s) == 1
            assert b <= cap or alone   # (a genome larger than the cap has a segment of its own)
        assert p["seg"][nd:] == sorted(p["seg"][nd:])


def test_staged_range_covers_every_byte_the_kmer_cutters_read(L):
    out = (C.c_int64 * 3)()
    rng = random.Random(5)
    for trial in range(2000):
        tb = rng.choice([0, 1, 3, 63, 64, 65, rng.randint(0, 1 << 27)])
        wl = rng.choice([1, 2, 31, 64, rng.randint(1, 200_000)])
        L.rh_stage_range(tb, wl, out)
        first, copy, total = out[0], out[1], out[2]
        b0, b1 = tb >> 2, (tb + wl - 1) >> 2   # bytes of the first and last base
        assert first % 16 == 0 and copy % 16 == 0 and total == copy + 32
        assert first <= b0 and b0 - first < 16
        assert first + copy > b1 and first + copy - (b1 + 1) < 16
        # aligned 64-bit words before the first base, the second word / five-dword gather behind the last: <= 20 bytes past it
        assert (b0 & ~7) >= first
        assert ((b1 & ~7) + 16) <= first + total and (b1 & ~3) + 20 <= first + total + 3
        # the copy never leaves the genome's pinned slot: a window ends inside the genome
        glen_bytes = b1 + 1 + rng.randint(0, 50)
        assert first + copy <= hslot(glen_bytes) - 16
