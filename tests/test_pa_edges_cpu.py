"""The named edges of the pseudo-alignment anchor stage without a GPU (tests/pa_cases.py, tests/pa_model.py):
  1. the model's own checks on every case: the literal radix tree of the oracle returns exactly the plain form's matches wherever
     some indexed k-mer shares p bases (asserted inside pa_model.model), the literal double loop equals the plain form on the
     small cases, the families are reached with their stated counts, a planted copy of p - 1 bases gives no anchor and one of
     p bases does;
  2. ClearSubstrPairs of the model equals the oracle's (lmo_clear_subs), and clear + trim of the model's raw list equals the
     anchors lmo_cmp_compare chains on the window text - whenever it returns them (it keeps them only when some survive the trim);
  3. necessity of the product's filter: every (window position, strand) that owns a model anchor passes lm_pa_candidate and, for
     p <= 15, lm_pa_candidate2, with the filter sized as the library sizes it for the query (queries on both sides of 16 414 bases);
  4. the product's search (lm_tree_search_first_tab + the enumeration up to `right`) returns the model's matches.
The window of 250 000 bases is not searched at every position in plain Python: pa_model asks the tree where the plain form matches
and where the partial-prefix rule can fire (its docstring says why that is all), and at every position of windows up to 6 000."""
import ctypes as C

import numpy as np
import pytest

import hostalgos as H
import oracle as O
import pa_cases as PC
import pa_model as M

K = 31


@pytest.fixture(scope="module")
def fx():
    f = PC.build()
    f["res"] = PC.run_models(f, brute_below=70)
    yield f
    for q in f["qindex"].values():
        q.close()


def test_cases_are_deterministic_and_well_formed(fx):
    again = PC.build()
    assert again["cases"] == fx["cases"] and again["genomes"] == fx["genomes"] and again["queries"] == fx["queries"]
    assert sorted(fx["calls"]["main"] + fx["calls"]["many"]) == list(range(len(fx["cases"])))
    assert [len(fx["calls"]["n%d" % n]) for n in (63, 64, 65, 129)] == [63, 64, 65, 129]
    for c in fx["cases"]:
        g = fx["genomes"][c.g][1][0][1]
        assert 0 <= c.tbegin and c.tbegin + c.wlen <= len(g) and c.qend <= len(fx["queries"][c.q])
    names = [c.name for c in fx["cases"]]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in fx["cases"]}
    assert by["first_genome_base0_rc0"].g == 0 and by["first_genome_base0_rc1"].tbegin == 0
    last = by["last_genome_last_base_rc1"]
    assert last.g == len(fx["genomes"]) - 1 and last.tbegin + last.wlen == len(fx["genomes"][-1][1][0][1])
    # the lane and slice boundaries the cases aim at are the kernel's: 64 / 65 positions are one / two positions per lane, 2048 /
    # 2049 positions one / two equal slices, 1920 / 1921 one / two strided slices
    assert PC.filter_slices(64, True) == [(0, 64, 1)] and PC.filter_slices(65, True) == [(0, 65, 2)]
    assert PC.filter_slices(2048, True) == [(0, 2048, 32)] and PC.filter_slices(2049, True) == [(0, 1025, 17), (1025, 2049, 16)]
    assert len(PC.filter_slices(1920, False)) == 1 and len(PC.filter_slices(1921, False)) == 2


def test_model_checks_and_reached_counters(fx):
    res = fx["res"]
    fam, tot = PC.check_reached(fx, res)
    print("pa edges, model:", tot)
    for f in sorted(fam):
        print("  %-12s %s" % (f, fam[f]))
    assert sum(r.counters["tree_checked"] for r in res.values()) > 20000
    # the minimum prefix of every length class, and what a planted copy gives on its own diagonal
    want_p = {9999: 11, 10000: 13, 49999: 13, 50000: 15, 249999: 15, 250000: 17}
    below = at = 0
    seen = set()
    for n, c in enumerate(fx["cases"]):
        r = res[n]
        if c.family == "pclass":
            assert r.p == want_p[c.wlen], c.name
        if len(fx["queries"][c.q]) < K or c.wlen < K:
            assert not r.raw, c.name
        for m, qp, wp in c.plants:
            if c.family in ("range", "qcontent"):
                continue  # (the query range cuts these on purpose: test below; low-complexity query k-mers are not indexed)
            on = [a for a in r.raw if a[3] == 0 and a[0] - a[1] == qp - wp and wp <= a[1] < wp + m and a[1] + a[2] <= wp + m]
            if m >= r.p:
                assert (qp, wp, min(m, K), 0, 0) in on, (c.name, m, qp, wp)
                assert len(on) == min(m - r.p, c.wlen - K - wp, len(fx["queries"][c.q]) - K - qp) + 1, (c.name, m, qp, wp, on)   # one per k-mer position of window and query that leaves >= p bases
                at += m == r.p
                seen.add((n, "p")) if m == r.p else None
            else:
                assert not on, (c.name, m, qp, wp, on)
                below += 1
                seen.add((n, "p-1")) if m == r.p - 1 else None
    assert below >= 40 and at >= 30
    for n, c in enumerate(fx["cases"]):   # in every length class, in both orientations: p - 1 bases give nothing, p bases an anchor
        if c.family == "pclass":
            assert (n, "p") in seen and (n, "p-1") in seen, c.name
    # reached: in every window above 95 bases an anchor is owned on both sides of every slice boundary of both filter forms and of
    # the first, a middle and the last lane boundary of every rolling slice (the strided 1919 | 1920 of 1951 ... 4127 included)
    kinds = {}
    for n, c in enumerate(fx["cases"]):
        if c.family == "wlen" and c.wlen > 95:
            own = {i for i, _ in res[n].owners}
            bs = PC.boundaries(c.wlen - K + 1, c.rc)
            assert sum(1 for k, _ in bs if k == "lane") >= 3, c.name
            for kind, x in bs:
                assert x in own and x + 1 in own, (c.name, kind, x)
                kinds[(kind, c.rc)] = kinds.get((kind, c.rc), 0) + 1
    print("  boundaries reached:", sorted(kinds.items()))   # three lane boundaries in each of the 8 rolling slices of the five lengths
    for rc in (0, 1):
        assert kinds[("lane", rc)] == 24 and kinds[("slice_roll", rc)] == 3 and kinds[("slice_strided", rc)] == 5
    by = {c.name: n for n, c in enumerate(fx["cases"])}
    for rc in (0, 1):
        assert not res[by["query_all_N_rc%d" % rc]].raw and not res[by["wlen_30_rc%d" % rc]].raw
        assert len(res[by["wlen_31_rc%d" % rc]].raw) >= 2   # the one position, both searches
        # a query k-mer that occurs three times: the window k-mers of the copy match three entries each
        r3 = res[by["kmer_three_times_rc%d" % rc]]
        assert sum(1 for k in r3.owners if sum(1 for a in r3.raw if a[1] == k[0] and a[3] == 0) >= 3) >= 10


def test_range_test_cases(fx):
    """forward search: the anchor at qbegin - 1 is skipped, the one at qbegin kept, one that ends at qend kept, at qend + 1 skipped;
    reverse search (other bounds): one that begins at qend is kept, at qend + 1 skipped, one that ends at qbegin kept, at qbegin - 1
    skipped"""
    res = fx["res"]
    by = {c.name: n for n, c in enumerate(fx["cases"])}
    for rc in (0, 1):
        def full(name, strand, qpos):
            return [a for a in res[by["range_%s_rc%d" % (name, rc)]].raw if a[4] == strand and a[2] == K and a[0] == qpos]
        assert full("qbegin", 0, 100) and not full("qbegin_minus_1", 0, 100) and full("qbegin_minus_1", 0, 101)
        assert full("qend_fwd", 0, 109) and not full("qend_fwd_plus_1", 0, 109) and full("qend_fwd_plus_1", 0, 108)
        assert full("rev_qend", 1, 309) and not full("rev_qend_plus_1", 1, 309) and full("rev_qend_plus_1", 1, 308)
        assert full("rev_qbegin", 1, 100) and not full("rev_qbegin_minus_1", 1, 100) and full("rev_qbegin_minus_1", 1, 101)


def _subs(anchors):
    arr = (O.Sub * max(len(anchors), 1))()
    for i, a in enumerate(anchors):
        arr[i].qbegin, arr[i].tbegin, arr[i].len, arr[i].trc, arr[i].qrc = a
    return arr


def _tuples(arr, n):
    return [(arr[i].qbegin, arr[i].tbegin, arr[i].len, arr[i].trc, arr[i].qrc) for i in range(n)]


def cmp_opt():
    opt = O.CmpOpt()
    opt.k, opt.min_prefix = 31, 11
    opt.c2.max_gap, opt.c2.min_score, opt.c2.min_align_len = 20, 35, 50
    opt.c2.min_identity, opt.c2.band_count, opt.c2.band_base, opt.c2.heuristic_pident = 70.0, 50, 100, 15.0
    return opt


def test_clear_equals_the_oracle(fx):
    L = O.lib()
    opt = cmp_opt()
    cmps = {}
    compared = with_chains = 0
    for n, c in enumerate(fx["cases"]):
        r = fx["res"][n]
        q = fx["queries"][c.q]
        arr = _subs(r.raw)
        m = L.lmo_clear_subs(arr, len(r.raw), K) if r.raw else 0
        assert _tuples(arr, m) == r.cleared, c.name
        if len(q) < K:
            continue
        if c.q not in cmps:
            cmps[c.q] = L.lmo_cmp_new(C.byref(opt))
            L.lmo_cmp_index(cmps[c.q], q, len(q))
        chains, subs, ns = C.POINTER(O.Chain2)(), C.POINTER(O.Sub)(), C.c_int(0)
        nc = L.lmo_cmp_compare(cmps[c.q], c.qbegin, c.qend, r.text, len(r.text), len(q), C.byref(chains), C.byref(subs), C.byref(ns))
        if ns.value:
            mt = L.lmo_trim_subs(arr, m, K, 100, None)
            assert _tuples(subs, ns.value) == _tuples(arr, mt), c.name
            compared += 1
            L.free(subs)
        else:
            assert m == 0 or L.lmo_trim_subs(arr, m, K, 100, None) == 0, c.name
        with_chains += nc > 0
        if nc:
            L.free(chains)
    for c in cmps.values():
        L.lmo_cmp_free(c)
    assert compared >= 140 and with_chains >= 10


def filter_log(qlen):
    """the size class of a query's prefix filter: the product's own rule (lm_pa_filter_log, which the query upload calls) for the
    2 (qlen - K + 1) entries the upload counts - both strands of every k-mer position, kept or not"""
    return H.lib().ha_pa_filter_log(2 * max(qlen - K + 1, 0))


def tab_bits(qlen):
    return H.lib().ha_cmp_tab_bits(2 * max(qlen - K + 1, 0))


def product_index(q):
    """the comparison index by the product's own primitives (k_extract_kmers: lm_revcomp, fwd == 0 || lm_low_complexity drop both
    strands of a position), sorted by (k-mer, value)"""
    Hh = H.lib()
    f, _ = M.kmers(q)
    out = []
    for x, k in enumerate(f.tolist()):
        if k == 0 or Hh.ha_low_complexity(k, K):
            continue
        out.append((k, x << 1))
        out.append((Hh.ha_revcomp(k, K), (x << 1) | 1))
    return sorted(out)


def test_filter_is_necessary_and_search_gives_the_models_matches(fx):
    Hh = H.lib()
    assert filter_log(16414) == 19 and filter_log(16415) == 20   # both sides of the LDS Bloom filter's reach
    owners = {19: 0, 20: 0, "other": 0}
    searched = 0
    tabs = {}
    for n, c in enumerate(fx["cases"]):
        r = fx["res"][n]
        if not r.matches:
            continue
        qi = fx["qindex"][c.q]
        qlen = len(fx["queries"][c.q])
        if c.q not in tabs:
            # the model's index is the product's (same k-mers kept, same values); the search below runs on the product's arrays
            pi = product_index(fx["queries"][c.q])
            assert pi == sorted(zip(qi.keys.tolist(), qi.vals.tolist())), "comparison index of query %d" % c.q
            keys = (C.c_uint64 * (len(pi) + 1))(*[k for k, _ in pi], 1 << 63)
            vals = [v for _, v in pi]
            lg, tb = filter_log(qlen), tab_bits(qlen)
            bits = (C.c_uint32 * int(Hh.ha_pa_bits_words(lg)))()
            Hh.ha_pa_filter_build(keys, len(pi), K, lg, bits)
            tab = (C.c_uint32 * ((1 << tb) + 1))()
            Hh.ha_build_tab(keys, len(pi), K, tb, tab)
            tabs[c.q] = (keys, vals, lg, bits, tb, tab)
        keys, vals, lg, bits, tb, tab = tabs[c.q]
        f, rcv = M.kmers(r.text)
        lo, hi = C.c_int(), C.c_int()
        for (i, strand), ms in r.matches.items():
            key = int((rcv if strand else f)[i])
            if (i, strand) in r.owners:
                assert Hh.ha_pa_candidate(bits, lg, key, r.p, K), (c.name, i, strand)
                if r.p <= 15:
                    assert Hh.ha_pa_candidate2(bits, lg, key, r.p, K), (c.name, i, strand)
                owners[lg if lg in owners else "other"] += 1
            if c.family == "many" and i % 16:
                continue  # (every 16th position of the tandem repeats: they are all alike)
            got = Hh.ha_tree_search_first_tab(keys, len(vals), key, r.p, K, tab, tb, C.byref(lo), C.byref(hi))
            # k-mer, common prefix (lm_lcp, as the enumeration of k_pa_search computes it) and value of every entry enumerated
            enum = sorted((keys[j], Hh.ha_lcp(keys[j], key, K), vals[j]) for j in range(lo.value, hi.value)) if got else []
            assert enum == sorted(ms), (c.name, i, strand)
            searched += 1
    print("filter necessity: owners by filter class", owners, "searches compared", searched)
    assert owners[19] > 50 and owners[20] > 50 and owners["other"] > 1000 and searched > 5000


def test_region_struct_matches_the_header(tmp_path):
    """lm_pa_region as Python declares it (api.PaRegion) has the size and the field offsets the C compiler gives the header's"""
    import os
    import subprocess
    from lexicmap_amd import api
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "r.c"
    fields = [f[0] for f in api.PaRegion._fields_]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lexicmap_hip.h"\nint main(void) { printf("%zu", sizeof(lm_pa_region));\n' +
                   "".join('printf(" %%zu", offsetof(lm_pa_region, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = str(tmp_path / "r")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [C.sizeof(api.PaRegion)] + [getattr(api.PaRegion, f).offset for f in fields]
