"""k_pa_filter with the rule map (lm_tune::pa_rule_map, LM_PA_RULE_MAP) on the GPU: the fixture of tests/pa_cases.py plus the windows
of tests/pa_rule_cases.py, which reach every branch of lm_pa_candidate3 on both strands, under a short query and one above 16 414
bases, at p = 11, 13 and 15.  Through Index.pseudoalign_regions, i.e. the kernels a search runs:
  * LM_PA_DROP_NESTED=0: the emitted anchor lists equal the model's raw lists exactly - with the rule map on and off, with the
    rolling and the strided form of the filter, on the device-resident and the host-resident handle;
  * default tuning: the two settings of the switch give identical lists."""
import pytest

import pa_cases as PC
import pa_rule_cases as RC

pytestmark = pytest.mark.gpu
CALLS = ("rule", "main", "three_queries")


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    import lexicmap_amd as la
    L = RC.shim(tmp_path_factory.mktemp("pa_rule_map"))
    f = RC.extend(PC.build(), L)
    bo = la.BuildOpt.default(masks=1024)
    f["dev"] = la.Index.from_genomes(f["genomes"], bo)
    f["host"] = la.Index.from_genomes(f["genomes"], bo, residency=la.api.Residency(la.api.GENOMES_HOST, 0))
    assert f["host"].residency()["genomes_host"] == len(f["genomes"]) and f["dev"].residency()["genomes_host"] == 0
    f["fetched"] = [f["dev"].fetch(g, 0, len(gs[1][0][1])) for g, gs in enumerate(f["genomes"])]
    f["res"] = PC.run_models(f)
    f["branches"] = RC.check_branches(f, f["res"], L)
    yield f
    f["dev"].close()
    f["host"].close()
    for q in f["qindex"].values():
        q.close()


def _call(fx, gi, call):
    idx = fx["calls"][call]
    cases = [fx["cases"][i] for i in idx]
    used = sorted({c.q for c in cases})
    qmap = {q: n for n, q in enumerate(used)}
    _, anchors = gi.pseudoalign_regions([fx["queries"][q] for q in used],
                                        [(qmap[c.q], c.qbegin, c.qend, c.g, c.tbegin, c.wlen, c.rc) for c in cases])
    return idx, anchors


def test_planted_windows_reach_every_branch(fx):
    print("rule-map branches, [keys, keys that own an anchor]:", sorted(fx["branches"].items()))
    ps = {fx["res"][n].p for n in fx["calls"]["rule"]}
    assert ps == {11, 13, 15}
    assert {fx["cases"][n].rc for n in fx["calls"]["rule"]} == {0, 1}


@pytest.mark.parametrize("handle", ["dev", "host"])
@pytest.mark.parametrize("roll", ["1", "0"])
@pytest.mark.parametrize("rule_map", ["1", "0"])
def test_emitted_equals_the_models_raw_list(fx, monkeypatch, handle, roll, rule_map):
    gi = fx[handle]
    monkeypatch.setenv("LM_PA_DROP_NESTED", "0")
    monkeypatch.setenv("LM_PA_FILTER_ROLL", roll)
    monkeypatch.setenv("LM_PA_RULE_MAP", rule_map)
    gi.tuning_reload()
    try:
        n = quirk = 0
        for call in CALLS:
            idx, anchors = _call(fx, gi, call)
            for i, got in zip(idx, anchors):
                r, c = fx["res"][i], fx["cases"][i]
                assert sorted(got) == sorted(r.raw), "%s, roll %s, rule map %s, case %s: %d emitted, %d in the model" % (
                    handle, roll, rule_map, c.name, len(got), len(r.raw))
                n += len(got)
                quirk += sum(1 for a in got if a[2] < r.p)
        assert n > 10000 and quirk > 100
    finally:
        for k in ("LM_PA_DROP_NESTED", "LM_PA_FILTER_ROLL", "LM_PA_RULE_MAP"):
            monkeypatch.delenv(k)
        gi.tuning_reload()


@pytest.mark.parametrize("handle", ["dev", "host"])
def test_default_tuning_same_lists_either_way(fx, monkeypatch, handle):
    gi = fx[handle]
    on = [_call(fx, gi, call) for call in CALLS]
    monkeypatch.setenv("LM_PA_RULE_MAP", "0")
    gi.tuning_reload()
    try:
        off = [_call(fx, gi, call) for call in CALLS]
    finally:
        monkeypatch.delenv("LM_PA_RULE_MAP")
        gi.tuning_reload()
    assert on == off
    assert sum(len(a) for _, anchors in on for a in anchors) > 5000
