"""The edge cases of base-level alignment and a checker of its result that needs no oracle.  Shared by
tests/test_wfa_edges_cpu.py (oracle, host-compiled device code, emulated forward pass) and tests/test_gpu_wfa_edges.py (kernels).

check_result(q, t, result) replays a run list over the two sequences, re-derives the score from the runs at the 4/6/2 penalties
and recomputes the coordinates and statistics the way oracle/lmo_wfa.c's header defines them.  cases() is the list of named
pairs: every one is built from a generator seeded by its own name, so a case is the same bytes wherever and in whatever order it
is made.  Lengths are the smallest that reach the path a group is about."""
import ctypes as C
import functools
import random
import zlib

import gotoh
import oracle as O

FIELDS = ("qbegin", "qend", "tbegin", "tend", "align_len", "matches", "gaps", "gap_regions")
DP_MAX = 12001   # the longest sequence the exact DP (and the oracle without wf-adaptive) is run on: 1.4e8 cells


# ---------------------------------------------------------------- references
def oracle_align(q, t, adaptive=1):
    """lmo_wfa_align as a record shaped like lexicmap_amd.Index.wfa's (status: None - the oracle has none)"""
    L = O.lib()
    r = O.WfaResult()
    assert L.lmo_wfa_align(q, len(q), t, len(t), adaptive, C.byref(r)) == 0
    res = dict(status=None, score=r.score, ops=[r.ops[i] for i in range(r.nops)])
    for f in FIELDS:
        res[f] = getattr(r, f)
    L.lmo_wfa_result_free(C.byref(r))
    return res


def same(a, b):
    """score, run list, coordinates and statistics of two records are equal (the status is not compared)"""
    return all(a[f] == b[f] for f in ("score", "ops") + FIELDS)


# ---------------------------------------------------------------- the run-list checker
def check_result(q, t, res):
    """res (status, score, ops as op << 32 | count, coordinates, statistics) is an alignment of q and t at its own score"""
    runs = [(chr(o >> 32), o & 0xFFFFFFFF) for o in res["ops"]]
    qp = tp = 0
    cost = 0
    prev = None
    for op, n in runs:
        assert n >= 1, ("empty run", op)
        assert op != prev, ("neighbouring runs of the same kind", op)
        prev = op
        if op == "M":
            assert q[qp:qp + n] == t[tp:tp + n] and qp + n <= len(q) and tp + n <= len(t), ("M run over unequal bytes", qp, tp, n)
            qp += n
            tp += n
        elif op == "X":
            assert qp + n <= len(q) and tp + n <= len(t), ("X run past an end", qp, tp, n)
            assert all(a != b for a, b in zip(q[qp:qp + n], t[tp:tp + n])), ("X run over equal bytes", qp, tp, n)
            qp += n
            tp += n
            cost += gotoh.MISMATCH * n
        elif op == "I":   # consumes target only
            tp += n
            cost += gotoh.GAP_OPEN + gotoh.GAP_EXTEND * n
        elif op == "D":   # consumes query only
            qp += n
            cost += gotoh.GAP_OPEN + gotoh.GAP_EXTEND * n
        else:
            raise AssertionError(("unknown op", op))
    assert (qp, tp) == (len(q), len(t)), ("the runs do not consume both sequences", qp, len(q), tp, len(t))
    assert res["score"] == cost, ("score is not the cost of the runs", res["score"], cost)
    # 1-based region between the first and the last M run, statistics over that region
    ms = [i for i, (op, _) in enumerate(runs) if op == "M"]
    exp = dict.fromkeys(FIELDS, 0)
    if ms:
        first, last = ms[0], ms[-1]
        qp = tp = 0
        for i, (op, n) in enumerate(runs):
            if i == first:
                exp["qbegin"], exp["tbegin"] = qp + 1, tp + 1
            if op in "MXD":
                qp += n
            if op in "MXI":
                tp += n
            if first <= i <= last:
                exp["align_len"] += n
                if op == "M":
                    exp["matches"] += n
                if op in "ID":
                    exp["gaps"] += n
                    exp["gap_regions"] += 1
            if i == last:
                exp["qend"], exp["tend"] = qp, tp
    assert {f: res[f] for f in FIELDS} == exp
    if res["status"] is not None:
        assert res["status"] == (0 if ms else 2), ("status", res["status"], "M runs", len(ms))


# ---------------------------------------------------------------- the cases
class Case:
    def __init__(self, group, name, q, t):
        self.group, self.name, self.q, self.t = group, name, bytes(q), bytes(t)

    @property
    def longest(self):
        return max(len(self.q), len(self.t))

    def __repr__(self):
        return "<%s %d/%d>" % (self.name, len(self.q), len(self.t))


def _rng(name):
    return random.Random(zlib.crc32(name.encode()))


def rand_seq(rng, n):
    return bytes(rng.choices(b"ACGT", k=n))


def other_base(rng, c):
    return rng.choice([x for x in b"ACGT" if x != c])


def substitute(rng, s, at):
    return s[:at] + bytes([other_base(rng, s[at])]) + s[at + 1:]


def mutate(rng, s, sub, ins, dele):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < dele:
            continue
        out.append(other_base(rng, c) if r < dele + sub else c)
        if rng.random() < ins:
            out.append(rng.choice(b"ACGT"))
    return bytes(out)


def _near_pair(rng, n):
    """a pair mutated at 2 % / 1 % / 1 % whose longer sequence has exactly n bases"""
    q = rand_seq(rng, n)
    return q, mutate(rng, q, 0.02, 0.01, 0.01)[:n]


TAIL_LENGTHS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
GROUPS = ("tails", "ties", "gaps", "many_runs", "bounds", "cells16", "long_bounds", "window", "outgrow", "nonacgt")


def _build():
    out = []

    def add(group, name, q, t):
        if len(q) and len(t):   # (zero-length sequences: the search never produces them)
            out.append(Case(group, name, q, t))

    # word and lane tails: pack16 packs 16 bases per word, a wavefront has 64 lanes
    for n in TAIL_LENGTHS:
        rng = _rng("tails-%d" % n)
        q = rand_seq(rng, n)
        add("tails", "tail%d-identical" % n, q, q)
        add("tails", "tail%d-del-middle" % n, q, q[:n // 2] + q[n // 2 + 1:])
        add("tails", "tail%d-sub-first" % n, q, substitute(rng, q, 0))
        add("tails", "tail%d-sub-last" % n, q, substitute(rng, q, n - 1))
        add("tails", "tail%d-first-missing" % n, q, q[1:])
        add("tails", "tail%d-last-missing" % n, q, q[:-1])
    rng = _rng("tails-1v40")
    one, forty = rand_seq(rng, 1), rand_seq(rng, 40)
    add("tails", "tail-1-vs-40", one, forty)
    add("tails", "tail-40-vs-1", forty, one)

    # ties: where the gap goes in a repeat is decided by the backtrace priority alone
    rng = _rng("ties")
    for label, unit, copies, fewer in (("A", b"A", 300, 287), ("AC", b"AC", 150, 143), ("ACG", b"ACG", 100, 96),
                                       ("37mer", rand_seq(rng, 37), 12, 10)):
        a, b = unit * copies, unit * fewer
        add("ties", "tie-%s-long-short" % label, a, b)
        add("ties", "tie-%s-short-long" % label, b, a)
        at = (len(a) // 2) | 1
        a2 = substitute(rng, a, at)   # one substitution inside the repeat
        add("ties", "tie-%s-sub-long-short" % label, a2, b)
        add("ties", "tie-%s-sub-short-long" % label, b, a2)

    # gaps: one gap at the start, in the middle, at the end, in either sequence; two gaps of opposite sign
    for g in (1, 2, 60, 300):
        rng = _rng("gap-%d" % g)
        q = rand_seq(rng, 500)
        for where, at in (("start", 0), ("middle", 250 - g // 2), ("end", 500 - g)):
            t = q[:at] + q[at + g:]
            add("gaps", "gap%d-%s-in-target" % (g, where), q, t)
            add("gaps", "gap%d-%s-in-query" % (g, where), t, q)
    for g in (5, 30):
        rng = _rng("gap-pair-%d" % g)
        q = rand_seq(rng, 500)
        t = q[:200] + q[200 + g:240 + g] + rand_seq(rng, g) + q[240 + g:]
        add("gaps", "gaps-opposite-%d" % g, q, t)

    # many runs: more runs than the ops estimate of the first pass (128 + 0.36 (qlen + tlen)); unrelated pairs
    for n in (1000, 2000):
        rng = _rng("alternate-%d" % n)
        q = rand_seq(rng, n)
        t = bytes(other_base(rng, c) if i & 1 else c for i, c in enumerate(q))
        add("many_runs", "alternate-%d" % n, q, t)
    for n in (150, 400):
        rng = _rng("unrelated-%d" % n)
        add("many_runs", "unrelated-%d" % n, rand_seq(rng, n), rand_seq(rng, n))

    # length-class bounds of wfa_batch (128 / 512 / 2048 / 4096 words of 16 bases) and the limit of the 16-bit cells
    for n in (2048, 2049, 8192, 8193):
        add("bounds", "bound-%d" % n, *_near_pair(_rng("bound-%d" % n), n))
    for n in (12000, 12001):
        add("cells16", "bound-%d" % n, *_near_pair(_rng("bound-%d" % n), n))
    for n in (32768, 32769, 65536, 65537):
        add("long_bounds", "bound-%d" % n, *_near_pair(_rng("bound-%d" % n), n))

    # the 4096-base window edge
    for n in (4095, 4096, 4097):
        add("window", "window-%d" % n, *_near_pair(_rng("window-%d" % n), n))
    rng = _rng("window-edit")
    q = rand_seq(rng, 5000)
    for at in (4095, 4096, 4097):
        add("window", "window-sub-at-%d" % at, q, substitute(rng, q, at))
    add("window", "window-del-at-4096", q, q[:4096] + q[4097:])

    # the final diagonal lies beyond the widest ring (1022 diagonals).  After an identical prefix that alone does not outgrow a
    # ring: every diagonal behind the gap's lags by more than wf-adaptive's 50 and is cut, the wavefront stays ~50 wide and the
    # ring is recentred under it (end-gap-1100-*: first ring).  The cut-off never closes the range TOWARDS the final diagonal,
    # so a pair that collects score on the way - 25 % divergence - is 1100 diagonals wide before it gets there (outgrow-*).
    rng = _rng("outgrow")
    q = rand_seq(rng, 200)
    t = q + rand_seq(rng, 1100)
    add("outgrow", "end-gap-1100-target-longer", q, t)
    add("outgrow", "end-gap-1100-query-longer", t, q)
    q = rand_seq(rng, 1500)
    t = mutate(rng, q, 0.25, 0.03, 0.03) + rand_seq(rng, 1100)
    add("outgrow", "outgrow-target-longer", q, t)
    add("outgrow", "outgrow-query-longer", t, q)

    # bytes that are not plain ACGT: compared as bytes by the fallback kernel
    rng = _rng("nonacgt")
    q = rand_seq(rng, 100)
    for at in (0, 15, 16, 99):
        add("nonacgt", "N-at-%d" % at, q[:at] + b"N" + q[at + 1:], q)
    add("nonacgt", "N-in-target-at-16", q, q[:16] + b"N" + q[17:])
    add("nonacgt", "N-both-same-column", q[:40] + b"N" + q[41:], q[:40] + b"N" + q[41:])
    add("nonacgt", "lower-case-query", q[:30] + q[30:50].lower() + q[50:], substitute(rng, q, 70))
    add("nonacgt", "lower-case-both", q.lower(), substitute(rng, q, 70).lower())
    q = rand_seq(rng, 8200)
    add("nonacgt", "N-at-5000-of-8200", q[:5000] + b"N" + q[5001:], q)

    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    assert {c.group for c in out} == set(GROUPS)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_build())


def by_group(group):
    return [c for c in cases() if c.group == group]


def by_name(name):
    return next(c for c in cases() if c.name == name)


# ---------------------------------------------------------------- shared references: computed once, never changed
@functools.lru_cache(maxsize=None)
def expected(name):
    """the oracle's result with wf-adaptive: what the reference computes"""
    c = by_name(name)
    return oracle_align(c.q, c.t, 1)


@functools.lru_cache(maxsize=None)
def dp_score(name):
    c = by_name(name)
    assert c.longest <= DP_MAX
    return gotoh.score(c.q, c.t)
