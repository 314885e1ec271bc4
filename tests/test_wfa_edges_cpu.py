"""Base-level alignment at its edges, without a GPU (the cases and the run-list checker: tests/wfa_cases.py).

The oracle's WFA (oracle/lmo_wfa.c) is a restatement of the published algorithm, and the device code was written against it: a
mistake the two share - a penalty, a tie rule, an end condition - no parity test sees.  So the oracle is held to an exact
three-matrix DP (tests/gotoh_host.cpp) and to a replay of its own run list, and then the product's host-compiled paths - ha_wfa
(lm_algos.h: the fallback kernel's algorithm) and the emulated forward pass of k_wfa_lean2 - to the oracle and the same checker."""
import ctypes as C

import pytest

import hostalgos as H
import wfa_cases as W
from test_wfa_lean2_emulated_cpu import run1

# cases whose wf-adaptive score differs from the exact one (the heuristic pruned the optimum).  At most 5 % of the cases may be
# listed; a case that joins the list is replaced rather than the cap raised.
ADAPTIVE_DIFFERS = ()

NAMES = [c.name for c in W.cases()]
DP_NAMES = [c.name for c in W.cases() if c.longest <= W.DP_MAX]
HOST_MAX = 2600   # the longest sequence the host-compiled device code is run on (the pairs that outgrow every ring: 2572)
HOST_NAMES = [c.name for c in W.cases() if c.longest <= HOST_MAX]


def test_the_case_list_is_what_the_paths_need():
    by = {g: W.by_group(g) for g in W.GROUPS}
    assert {c.longest for c in by["bounds"] + by["cells16"] + by["long_bounds"]} == {2048, 2049, 8192, 8193, 12000, 12001, 32768, 32769, 65536, 65537}
    assert {c.longest for c in by["window"]} >= {4095, 4096, 4097, 5000}
    for c in by["outgrow"]:
        assert abs(len(c.t) - len(c.q)) > 1022 and c.longest <= HOST_MAX
    for c in by["nonacgt"]:
        assert set(c.q + c.t) - set(b"ACGT")
    for c in W.cases():
        if c.group != "nonacgt":
            assert not set(c.q + c.t) - set(b"ACGT"), c.name
    for n in (1000, 2000):   # more runs than the first pass's ops estimate (est_div 0.12 without a pseudo-alignment)
        c = W.by_name("alternate-%d" % n)
        assert len(W.expected(c.name)["ops"]) > 128 + 3.0 * 0.12 * (len(c.q) + len(c.t))
    assert len(ADAPTIVE_DIFFERS) <= 0.05 * len(NAMES) and set(ADAPTIVE_DIFFERS) <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_an_alignment_at_the_dp_optimum(name):
    c = W.by_name(name)
    adaptive = W.expected(name)
    W.check_result(c.q, c.t, adaptive)
    if c.longest > W.DP_MAX:
        return
    dp = W.dp_score(name)
    exact = W.oracle_align(c.q, c.t, 0)
    assert exact["score"] == dp
    W.check_result(c.q, c.t, exact)
    assert adaptive["score"] >= dp
    assert (adaptive["score"] != exact["score"]) == (name in ADAPTIVE_DIFFERS)


def _ha_wfa(q, t):
    """lm_wfa_align on the host with the retry protocol of the pipeline's fallback: status 1 doubles the score bound"""
    max_score, arena = 64, 1 << 12
    while True:
        ops = (C.c_uint64 * (len(q) + len(t) + 8))()
        out = H.WfaOut()
        st = H.lib().ha_wfa(q, len(q), t, len(t), max_score, arena, ops, len(ops), C.byref(out))
        if st != 1:
            break
        assert max_score <= 8 * (len(q) + len(t)) + 64   # a global alignment never costs more
        max_score *= 2
        arena *= 4
    res = dict(status=st, score=out.score, ops=[ops[i] for i in range(out.nops)])
    for f in W.FIELDS:
        res[f] = getattr(out, f)
    return res


@pytest.mark.parametrize("name", HOST_NAMES)
def test_host_compiled_wfa(name):
    c = W.by_name(name)
    got = _ha_wfa(c.q, c.t)
    assert got["status"] in (0, 2)
    W.check_result(c.q, c.t, got)
    assert W.same(got, W.expected(name))
    assert got["score"] >= W.dp_score(name)
    if name not in ADAPTIVE_DIFFERS:
        assert got["score"] == W.dp_score(name)


def _emulated(c, exp, nc, r16, win, last_nc=16):
    """the forward pass at the given width; status 3 goes to the next width as in wfa_batch -> the last pass's record"""
    smax = exp["score"] + 16
    while True:
        arena = (smax // 2 + 2) * 64 * nc + 2 * (len(c.q) + len(c.t)) + 4096
        st, got, _ = run1(c.q, c.t, nc, r16 and nc <= 4, max_score=smax, arena_cap=arena, win=win)
        if st != 3 or got[1] == 0 or nc >= last_nc:   # (status 3 with score 0: not plain ACGT - no width helps)
            break
        nc *= 2
    res = dict(status=st, score=got[1], ops=got[2])
    res.update(zip(W.FIELDS, got[3:]))
    return res


@pytest.mark.parametrize("nc,r16,win", [(1, False, False), (1, True, False), (2, False, False), (2, True, False), (4, False, False),
                                        (4, True, False), (1, False, True), (2, False, True), (4, False, True)])
@pytest.mark.parametrize("group", [g for g in W.GROUPS if any(c.longest <= HOST_MAX for c in W.by_group(g))])
def test_emulated_forward_pass(group, nc, r16, win):
    n = 0
    for c in W.by_group(group):
        if c.longest > HOST_MAX:
            continue
        exp = W.expected(c.name)
        if c.name.startswith("outgrow-"):
            # wider than every ring: each pass up to the 1024-diagonal one says so (status 3 and the width it would have
            # needed) and the fallback takes the pair.  The 512- and 1024-diagonal passes have no 16-bit cells and do not
            # depend on where the chain began: they run once per form, from the 256-diagonal start
            last = 16 if (nc, r16) == (4, False) else 4
            got = _emulated(c, exp, nc, r16, win, last_nc=last)
            assert got["status"] == 3 and got["score"] > 64 * last - 2, c.name
            n += 1
            continue
        got = _emulated(c, exp, nc, r16, win)
        if group == "nonacgt":       # left to the byte-comparing fallback (test_host_compiled_wfa)
            assert (got["status"], got["score"]) == (3, 0), c.name
        else:
            assert got["status"] in (0, 2), (c.name, got["status"], got["score"])
            W.check_result(c.q, c.t, got)
            assert W.same(got, exp), c.name
        n += 1
    assert n > 0
