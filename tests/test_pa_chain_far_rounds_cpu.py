"""The candidate rounds of pa_chain_dp_reg (lm_pa_chain_dp_core.h) behind the first 64 anchors - the LDS ring (up to PCD_RING =
128 anchors back) and global memory beyond it - run only while the band of Chainer2 has not closed.  The band closes once it
is wider than band_base = --align-band bases AND holds more than band_count = --align-band / 2 candidates
(lib-chaining2.go:222-307), so at the default of 100 the first round is nearly always the only one.

indel_windows() builds the pseudo-alignment windows that tests/test_gpu_search_options.py sends to the device for the
non-default --align-band / --align-max-gap values.  Here, without a GPU, the oracle's anchors of those windows (after
ClearSubstrPairs + Trim, the list lmo_cmp_compare hands to Chainer2) are shown to reach both far rounds, with predecessors
chosen more than 64 anchors back, and the emulated kernel DP is checked against lm_run_chain2 on them."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from lexicmap_amd import synth
from test_pa_chain_emulated_cpu import lib as emu_lib


def indel_rich(rng, s, sub=0.05, every=(300, 500), indel=(30, 91)):
    """s (uint8 array) with `sub` substitutions and one insertion or deletion of 30-90 bp every ~400 bp"""
    s = synth.mutate(rng, s, sub=sub)
    out, pos = [], 0
    while pos < len(s):
        step = int(rng.integers(*every))
        out.append(s[pos:pos + step])
        pos += step
        n = int(rng.integers(*indel))
        if rng.random() < 0.5:
            out.append(synth.random_seq(rng, n))
        else:
            pos += n
    return np.concatenate(out)


def indel_windows(seed=91, nq=8, qlen=3000, flank=300):
    """queries: random 3-kb sequences; problems (query index, qbegin, qend, window): two independent indel-rich copies of
    each query, between random flanks"""
    rng = np.random.default_rng(seed)
    queries, problems = [], []
    for qi in range(nq):
        q = synth.random_seq(rng, qlen)
        queries.append(q.tobytes())
        for _ in range(2):
            w = np.concatenate([synth.random_seq(rng, flank), indel_rich(rng, q), synth.random_seq(rng, flank)])
            problems.append((qi, 0, qlen - 1, w.tobytes()))
    return queries, problems


def cmp_opt(align_band=100, align_max_gap=20, align_min_match_len=50, align_min_pident=70.0):
    """SeqComparatorOptions as search.go:364-383 sets them from the flags"""
    o = O.CmpOpt()
    o.k, o.min_prefix = 31, 11
    o.c2.max_gap = align_max_gap
    o.c2.min_score = int(align_min_match_len * align_min_pident / 100)
    o.c2.min_align_len = align_min_match_len
    o.c2.min_identity = align_min_pident
    o.c2.band_base, o.c2.band_count = align_band, align_band // 2
    o.c2.heuristic_pident = 15.0
    o.min_aligned_fraction, o.min_identity = 0.0, align_min_pident
    return o


def oracle_anchors(queries, problems, opt):
    """per problem: (the oracle's chains - qbegin, qend, tbegin, tend, nanchors, matched_bases, aligned_bases_q,
    aligned_bases_t, pident - and the cleared + trimmed anchors it chained)"""
    L = O.lib()
    out, cache = [], {}
    for qi, qb, qe, t in problems:
        if qi not in cache:
            c = L.lmo_cmp_new(C.byref(opt))
            L.lmo_cmp_index(c, queries[qi], len(queries[qi]))
            cache[qi] = c
        chains, subs, ns = C.POINTER(O.Chain2)(), C.POINTER(O.Sub)(), C.c_int()
        nc = L.lmo_cmp_compare(cache[qi], qb, qe, t, len(t), len(queries[qi]), C.byref(chains), C.byref(subs), C.byref(ns))
        ch = [(chains[i].qbegin, chains[i].qend, chains[i].tbegin, chains[i].tend, chains[i].nanchors,
               chains[i].matched_bases, chains[i].aligned_bases_q, chains[i].aligned_bases_t, chains[i].pident)
              for i in range(nc)]
        an = [(subs[i].qbegin, subs[i].tbegin, subs[i].len) for i in range(ns.value)]
        if nc:
            L.free(chains)
        if ns.value:
            L.free(subs)
        out.append((ch, an))
    for c in cache.values():
        L.lmo_cmp_free(c)
    return out


def scan_depth(a, i, band_base, band_count):
    """how many anchors before anchor i the candidate scan of Chainer2 looks at before the band closes (i if it never does)"""
    aq, at = a[i][0], a[i][1]
    cnt = 0
    for j in range(i - 1, -1, -1):
        bq, bt, bl = a[j]
        if bq == aq or bt > at:
            continue
        cnt += 1
        if not (aq - bq - bl <= band_base or cnt <= band_count):
            return i - j
    return i


BANDS = [(100, 20), (140, 20), (400, 20), (400, 100), (1000, 100)]


@pytest.fixture(scope="module")
def windows():
    return indel_windows()


def test_windows_have_the_size_the_calibration_expects(windows):
    queries, problems = windows
    res = oracle_anchors(queries, problems, cmp_opt())
    sizes = [len(an) for _, an in res]
    assert min(sizes) >= 300, sizes
    assert all(len(ch) >= 2 for ch, _ in res)   # the indels split every window into several chains at the defaults


@pytest.mark.parametrize("band,max_gap", BANDS)
def test_the_band_reaches_the_ring_and_global_rounds(windows, band, max_gap):
    """restates the band-closing rule on the oracle's anchors: which rounds of pa_chain_dp_reg each anchor needs"""
    queries, problems = windows
    res = oracle_anchors(queries, problems, cmp_opt(band, max_gap))
    depth = [scan_depth(an, i, band, band // 2) for _, an in res for i in range(len(an))]
    n, ring, glob = len(depth), sum(d > 64 for d in depth), sum(d > 128 for d in depth)
    if band == 100:
        # the default: the registers hold the band of most anchors
        assert ring < n // 5 and glob < n // 100, (n, ring, glob)
    elif band == 140:
        # 70 candidates: most anchors need the LDS ring, a few go past it
        assert ring > n // 2 and 0 < glob < n // 20, (n, ring, glob)
    else:
        # 200 / 500 candidates: most anchors read candidates from global memory
        assert glob > n // 2, (n, ring, glob)


@pytest.mark.parametrize("band,max_gap", BANDS)
def test_far_predecessors_and_the_emulated_kernel_dp(windows, band, max_gap):
    """the DP of the kernel (host SIMT emulator) equals lm_run_chain2 on every window, every msi (score << 32 | predecessor)
    included, and msi is then read back from it: for the wide bands some chosen predecessor lies in the ring or beyond it, so a wrong far round would change a score"""
    queries, problems = windows
    res = oracle_anchors(queries, problems, cmp_opt(band, max_gap))
    far = []
    for _, an in res:
        n = len(an)
        qb = (C.c_int32 * n)(*[a[0] for a in an])
        tb = (C.c_int32 * n)(*[a[1] for a in an])
        ln = (C.c_uint8 * n)(*[a[2] for a in an])
        msi = (C.c_uint64 * n)()
        M, Mi = C.c_longlong(), C.c_int()
        assert emu_lib().pcd_emu_check(qb, tb, ln, n, max_gap, band, band // 2, msi, C.byref(M), C.byref(Mi)) == 0
        far.append(max(i - (msi[i] & 0xffffffff) for i in range(n)))
    if band == 140:
        assert max(far) > 64, far
    elif (band, max_gap) in ((400, 20), (1000, 100)):
        assert max(far) > 128, far
