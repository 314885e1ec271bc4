"""The nested-anchor rule of the pseudo-alignment without a GPU (lm_pa_anchor_nested, lm_algos.h): k_pa_search
does not emit an anchor when the neighbouring window position of the same exact-match run emits its container.  For chain
windows cut from mutated copies of a query, tests/pa_nested_host.cpp enumerates the raw anchors with a plain model and with
the kernel's own search, and checks that
  1. every anchor the predicate marks has its container in the raw list, and
  2. lm_clear_sorted over the raw list equals lm_clear_sorted over the list without the marked anchors, element for element.
The shapes at which the rule could go wrong are built on purpose and counted."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = 31

COUNTERS = ("raw", "nested", "cleared", "fwd_nested", "rev_nested", "win_pos0", "qbegin", "rev_last", "run31", "run32", "run40",
            "lp_p1", "q_lowc", "q_n", "quirk", "no_prev", "len_k")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pa_nested") / "libpa_nested_host.so")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fPIC", "-shared",
                           "-o", so, os.path.join(HERE, "pa_nested_host.cpp")])
    L = C.CDLL(so)
    L.pn_case.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int] + [C.c_int] * 8 + [C.POINTER(C.c_longlong), C.c_char_p, C.c_int]
    assert L.pn_ncounters() == len(COUNTERS)
    return L


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, s, div):
    """substitutions, insertions and deletions at rate `div` (2 : 1 : 1)"""
    out = []
    for c in s:
        r = rng.random()
        if r < div * 0.5:
            out.append(rng.choice([b for b in "ACGT" if b != c]))
        elif r < div * 0.75:
            out.append(c + rng.choice("ACGT"))
        elif r < div:
            pass
        else:
            out.append(c)
    return "".join(out)


def substitute(s, at):
    s = list(s)
    for a in at:
        s[a] = {"A": "C", "C": "G", "G": "T", "T": "A", "N": "C"}[s[a]]
    return "".join(s)


def run(lib, totals, q, g, tbegin, wlen, wrc, p, qb, qe, index_k=K):
    cnt = (C.c_longlong * len(COUNTERS))()
    err = C.create_string_buffer(400)
    rc = lib.pn_case(q.encode(), len(q), g.encode(), len(g), tbegin, wlen, int(wrc), K, index_k, p, qb, qe, cnt, err, 400)
    assert rc == 0, "%s (query %d bases, window [%d, +%d) rc %d, p %d, query range [%d, %d], index k %d)" % (
        err.value.decode(), len(q), tbegin, wlen, wrc, p, qb, qe, index_k)
    got = dict(zip(COUNTERS, cnt))
    for k, v in got.items():
        totals[k] = totals.get(k, 0) + v
    return got


def window(g, a, b, wrc):
    """(genome, tbegin, wlen) whose window reads g[a:b]: the range itself, or the same range of the other strand (the search
    turns a window whose seeds matched on the other strand round, so a window always reads along the query)"""
    return (revcomp(g), len(g) - b, b - a) if wrc else (g, a, b - a)


def need(got, *names):
    for k in names:
        assert got[k] > 0, "no case of '%s': %s" % (k, sorted(got.items()))


def test_nested_anchors_have_containers_and_clear_is_unchanged(lib):
    rng = random.Random(20240611)
    totals = {}
    # ---- random queries against windows cut from mutated copies: divergence 0-15 %, both window orientations, windows that
    # start and end inside the copy, a query range inside the query
    for n, (qlen, div) in enumerate([(200, 0.0), (450, 0.03), (900, 0.06), (1500, 0.10), (2200, 0.15), (3000, 0.05), (1200, 0.0),
                                     (700, 0.08)]):
        q = rand_seq(rng, qlen)
        for wrc in (0, 1):
            copy = mutate(rng, q, div)
            left, right = rand_seq(rng, rng.randint(0, 300)), rand_seq(rng, rng.randint(40, 300))
            g = left + copy + right
            cut = rng.randint(0, 1)  # the window starts / ends inside the copy, or holds it whole
            tbegin = len(left) + rng.randint(5, 60) if cut else rng.randint(0, len(left))
            tend = len(left) + len(copy) - rng.randint(5, 60) if cut else len(left) + len(copy) + rng.randint(0, 40)
            qb = rng.randint(0, qlen // 4)
            qe = qlen - rng.randint(0, qlen // 4)
            got = run(lib, totals, q, *window(g, tbegin, tend, wrc), wrc, (11, 13, 15)[n % 3], qb, qe)
            need(got, "raw")
    # ---- exact runs of 31, 32 and 40 bases between substitutions; a run that starts the window; a run that starts at QBegin
    q = rand_seq(rng, 600)
    marks = [100, 132, 165, 206, 300, 400]
    g = rand_seq(rng, 64) + substitute(q, marks) + rand_seq(rng, 64)
    for wrc in (0, 1):
        got = run(lib, totals, q, *window(g, 0, len(g), wrc), wrc, 11, 0, len(q))
        need(got, "run31", "run32", "run40")
        # the window starts 20 bases before the substitution at 300 and the query range 18 bases before the one at 400, both
        # inside a run: the anchors there are shorter than K and their containers lie outside
        got = run(lib, totals, q, *window(g, 64 + 280, len(g), wrc), wrc, 13, 0, len(q))
        need(got, "win_pos0")
        got = run(lib, totals, q, *window(g, 64 + 280, len(g), wrc), wrc, 13, 382, 560)
        need(got, "qbegin")
    # ---- the last window position in the reverse-strand search (common suffixes): the window ends 20 bases behind the
    # substitution at 300, inside a run
    for wrc in (0, 1):
        got = run(lib, totals, q, *window(g, 0, 64 + 300 + 1 + 20, wrc), wrc, 11, 0, len(q))
        need(got, "rev_last", "rev_nested")
    # ---- low-complexity query k-mers (poly-A, a dinucleotide repeat) right before and after runs; an N in the query next to a run
    q = rand_seq(rng, 300) + "A" * 45 + rand_seq(rng, 200) + "AT" * 24 + rand_seq(rng, 200)
    qn = list(q)
    for at in (120, 121, 400, 650):
        qn[at] = "N"
    qn = "".join(qn)
    for wrc in (0, 1):
        g = rand_seq(rng, 30) + q + rand_seq(rng, 30)
        got = run(lib, totals, qn, *window(g, 0, len(g), wrc), wrc, 11, 0, len(qn))
        need(got, "q_lowc", "q_n")
    # ---- an index whose k is not the comparison's (k = 21): the comparison index is written twice, K stays 31
    q = rand_seq(rng, 800)
    g = rand_seq(rng, 100) + mutate(rng, q, 0.04) + rand_seq(rng, 100)
    got = run(lib, totals, q, g, 0, len(g), 0, 11, 0, len(q), index_k=21)
    need(got, "nested")
    got = run(lib, totals, q, *window(g, 0, len(g), 1), 1, 13, 0, len(q), index_k=21)
    need(got, "nested")

    print("pa nested totals:", totals)
    need(totals, "raw", "nested", "cleared", "fwd_nested", "rev_nested", "win_pos0", "qbegin", "rev_last", "run31", "run32", "run40",
         "lp_p1", "q_lowc", "q_n", "no_prev", "len_k")
    assert totals["nested"] < totals["raw"] and totals["cleared"] <= totals["raw"] - totals["nested"]


def test_the_kernel_and_the_test_share_one_statement_of_the_rule():
    csrc = os.path.join(ROOT, "lexicmap_amd", "csrc")
    algos = open(os.path.join(csrc, "lm_algos.h")).read()
    kern = open(os.path.join(csrc, "lm_kernels.hip")).read()
    assert "LM_HD bool lm_pa_anchor_nested(" in algos
    # the kernel evaluates the predicate's two halves (window side once per candidate, match side once per match)
    assert "lm_pa_nested_window(" in kern and "lm_pa_nested_match(" in kern and "lm_cmp_vals(" in kern
    body = algos[algos.index("LM_HD bool lm_pa_anchor_nested("):]
    body = body[:body.index("\n}\n")]
    assert "lm_pa_nested_match(" in body and "lm_pa_nested_window(" in body
