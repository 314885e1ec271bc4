"""Seed lookup, anchor assembly, ClearSubstrPairs and Chainer.Chain on indexes of tiny genomes, without a GPU: the oracle
against the plain model of seed_model.py on every case of seed_cases.py, the coverage the cases must give (conditions on the
INPUTS, asserted from the model, so that the GPU test of the same cases cannot pass while checking nothing), and the host
build of the device's lm_clear_sorted / lm_run_chain1 against the oracle on every pair of the cases.
"""
import ctypes as C

import numpy as np
import pytest

import hostalgos as H
import oracle as O
import seed_cases as SC
import seed_model as SM
from test_device_algos_cpu import gap_lut

NAMES = list(SC.INDEXES)
SETS = ("default", "p_lo", "p_k")
MAX_GAP, MAX_DISTANCE = SC.MAX_GAP, SC.MAX_DISTANCE

_cases = {}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("seed_edges"))

    def get(name):
        if name not in _cases:
            _cases[name] = SC.Case(name, d)
        return _cases[name]
    yield get
    _cases.clear()


@pytest.mark.parametrize("oname", SETS)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_anchors_equal_the_plain_model(case, name, oname):
    """lmo_stage_anchors, sorted per genome = every stored seed in range and direction that the start rule does not lose,
    once per query location"""
    c = case(name)
    s = c.set(oname)
    total = 0
    for qi, qn in enumerate(c.names):
        exp, got = s["model"][qi], s["oracle"][qi]
        assert sorted(exp) == sorted(got), (qn, sorted(set(exp) ^ set(got))[:5])
        for g in exp:
            assert np.array_equal(SM.sorted_rows(got[g]), exp[g]), (qn, g, len(got[g]), len(exp[g]))
            total += len(exp[g])
        if qn in ("too_short", "all_N"):
            assert not got
    assert total > 1000


def test_the_cases_reach_the_edges_they_were_made_for(case):
    last = {n: 4 ** case(n).lists.a - 1 for n in NAMES}
    facts = {(n, o): case(n).set(o)["facts"] for n in NAMES for o in SETS}
    count = lambda cond: sum(int(cond(f, n).sum()) for (n, _o), f in facts.items())
    lost = {k: int(f["lost"].sum()) for k, f in facts.items()}
    print("lookups lost to the start rule:", lost)
    assert count(lambda f, n: f["lost"]) >= 10
    for n in NAMES:  # (and in every index, at its defaults)
        assert lost[(n, "default")] >= 10, n
    assert count(lambda f, n: f["outlier"] & (f["nvalues"] > 0) & ~f["lost"]) >= 100
    assert count(lambda f, n: f["nvalues"] >= 65) >= 1
    assert count(lambda f, n: f["outlier"] & (f["nvalues"] >= 65) & ~f["lost"]) >= 1      # out_vals spread over a wavefront
    assert count(lambda f, n: (f["nloc"] >= 2) & (f["nvalues"] > 0)) >= 1
    assert count(lambda f, n: (f["nloc"] >= 2) & (f["nvalues"] >= 65) & ~f["lost"]) >= 1
    assert count(lambda f, n: (f["nloc"] >= 2) & (f["nvalues"] > 0) & f["outlier"] & ~f["lost"]) >= 1
    assert count(lambda f, n: ~f["outlier"] & (f["partition"] == 0) & (f["nvalues"] > 0)) >= 1
    assert count(lambda f, n: ~f["outlier"] & (f["partition"] == last[n]) & (f["nvalues"] > 0)) >= 1
    assert count(lambda f, n: f["empty_partition"]) >= 1
    assert count(lambda f, n: f["dropped"]) >= 1
    # both prefix lengths at their bounds change what is found
    for n in NAMES:
        a = {o: sum(len(r) for per in case(n).set(o)["oracle"] for r in per.values()) for o in SETS}
        assert a["p_lo"] > a["default"] >= a["p_k"] > 0, (n, a)
    # chaining: the targeted pair sizes, on the large genome of V20k
    c = case("V20k")
    sizes = {qn: len(per.get(SC.genome_key(0), ())) for qn, per in zip(c.names, c.set("default")["oracle"])}
    for t in SC.CHAIN_TARGETS:
        assert sizes["pair%d" % t] == t
    assert sizes["pair65_rc"] == 65 and sizes["pair129_rc"] == 129
    assert 300 <= sizes["pair_mid"] <= 500
    assert max(len(r) for r in c.set("default")["oracle"][c.names.index("tiny_1k_whole")].values()) >= 10000
    both = several = 0
    for n in NAMES:
        for per in case(n).chained("default"):
            for raw, cleared, _score, chains in per.values():
                signs = {int(np.sign(cleared[b, 1] - cleared[a, 1])) for ch in chains for a, b in zip(ch, ch[1:])}
                both += {1, -1} <= signs
                several += len(chains) >= 2
    assert both >= 1 and several >= 1


def _subs(rows):
    a = (H.Sub * max(len(rows), 1))()
    v = np.frombuffer(a, dtype=SC.SUB_DTYPE)[:len(rows)]
    v["qbegin"], v["tbegin"], v["len"], v["qrc"], v["trc"] = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4]
    return a, v


@pytest.mark.parametrize("oname", ("default", "p_k"))
@pytest.mark.parametrize("name", NAMES)
def test_host_clear_and_chain_equal_the_oracle_on_every_pair(case, name, oname):
    """lm_clear_sorted and lm_run_chain1 (what k_chain1 runs per lane, built for the host) against lmo_clear_subs and
    lmo_chainer: cleared anchors, score bits and chains"""
    c = case(name)
    L, Hh = O.lib(), H.lib()
    min_score = L.lmo_seed_weight(float(c.set(oname)["min_single_prefix"]))
    lut = gap_lut(64)
    npairs = 0
    for qn, per in zip(c.names, c.chained(oname)):
        for g, (raw, cleared, score, chains) in per.items():
            n = len(raw)
            da, view = _subs(raw)
            nd = Hh.ha_clear_sorted(da, n, c.k) if n > 1 else n
            assert nd == len(cleared), (qn, g)
            got = np.stack([view[f][:nd].astype(np.int64) for f in SC.FIELDS], axis=1)
            assert np.array_equal(got, cleared), (qn, g)
            doff = (C.c_int32 * (nd + 4))()
            didx = (C.c_int32 * (2 * nd + 6))()
            dn = C.c_int()
            sd = Hh.ha_chain1(da, nd, MAX_GAP, min_score, MAX_DISTANCE, 0, lut, len(lut), doff, didx, C.byref(dn))
            assert np.float32(sd).tobytes() == np.float32(score).tobytes(), (qn, g)
            assert [[didx[j] for j in range(doff[x], doff[x + 1])] for x in range(dn.value)] == chains, (qn, g)
            npairs += 1
    assert npairs >= 5


def _gap(a, b):  # lib-chaining.go:655-660
    dq = abs(int(a[0] - b[0]))
    dt = abs(int(a[1] - b[1])) if a[1] >= b[1] else abs(int(a[1] + a[2] - b[1] - b[2]))
    return abs(dq - dt)


@pytest.mark.parametrize("name", NAMES)
def test_cleared_anchors_and_chains_are_well_formed(case, name):
    """what ClearSubstrPairs and Chainer.Chain promise, checked on the oracle's results without restating either: the cleared
    anchors are a subsequence of the raw ones and every dropped one lies inside an earlier raw one; chains are ascending lists
    of cleared anchors that share no anchor (but for the first member of a chain cut at a change of direction, which belongs
    to the chain before the change as well); a pair has chains exactly if its best score reaches the minimum; consecutive
    members lie within --seed-max-dist and --seed-max-gap"""
    c = case(name)
    min_score = O.lib().lmo_seed_weight(float(c.set("default")["min_single_prefix"]))
    ndropped = nlinks = 0
    for qn, per in zip(c.names, c.chained("default")):
        for g, (raw, cleared, score, chains) in per.items():
            # subsequence
            keep = np.zeros(len(raw), dtype=bool)
            j = 0
            for i in range(len(raw)):
                if j < len(cleared) and np.array_equal(raw[i], cleared[j]):
                    keep[i] = True
                    j += 1
            assert j == len(cleared), (qn, g)
            # a dropped anchor equals or lies inside an earlier raw one (an anchor equal to an earlier one stands for it)
            first = np.ones(len(raw), dtype=bool)
            first[1:] = (raw[1:, :3] != raw[:-1, :3]).any(axis=1)
            fi = np.flatnonzero(first)
            u = raw[fi]
            qe, te = u[:, 0] + u[:, 2], u[:, 1] + u[:, 2]
            for x in np.flatnonzero(~keep):
                if not first[x]:
                    ndropped += 1
                    continue
                y = int(np.searchsorted(fi, x))
                inside = (u[:y, 0] <= raw[x, 0]) & (qe[:y] >= raw[x, 0] + raw[x, 2]) & (u[:y, 1] <= raw[x, 1]) & \
                         (te[:y] >= raw[x, 1] + raw[x, 2])
                assert inside.any(), (qn, g, x)
                ndropped += 1
            # chains
            assert (len(chains) > 0) == (score >= min_score), (qn, g, score)
            owned = []
            for ch in chains:
                assert len(ch) >= 1 and all(0 <= i < len(cleared) for i in ch)
                assert all(a < b for a, b in zip(ch, ch[1:]))
                owned += ch[1:] if len(ch) > 1 else ch
                for a, b in zip(ch, ch[1:]):
                    A, B = cleared[b], cleared[a]
                    assert A[0] - B[0] <= MAX_DISTANCE and abs(A[1] - B[1]) <= MAX_DISTANCE and _gap(A, B) <= MAX_GAP
                    nlinks += 1
            assert len(owned) == len(set(owned)), (qn, g)
    assert ndropped > 100 and nlinks > 100
