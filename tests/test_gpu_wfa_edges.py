"""The WFA kernels at their edges (the cases and the run-list checker: tests/wfa_cases.py; the same cases without a GPU:
tests/test_wfa_edges_cpu.py).  Every pair goes through lm_wfa_batch (la.Index.wfa) under the default tuning and under each
switch that forces another instantiation; the result must equal the oracle's in every field, replay as an alignment of the two
sequences at its own score, and - up to 12 001 bases - cost what an exact affine-gap DP says is the optimum.  The profile says
which kernels a group went through: the fallback kernel, the 1024-diagonal ring and the windowed forms are reached on purpose."""
import pytest

import lexicmap_amd as la
import oracle as O
import wfa_cases as W
from lexicmap_amd import synth
from test_wfa_edges_cpu import ADAPTIVE_DIFFERS

pytestmark = pytest.mark.gpu

SWITCHES = ("LM_WFA_FIRST_NC", "LM_WFA_R16", "LM_WFA_WIN")
SETTINGS = {"default": {}, "first_nc_1": {"LM_WFA_FIRST_NC": "1,1,1,1,1"}, "r16_off": {"LM_WFA_R16": "0"},
            "win_all": {"LM_WFA_WIN": "11111"}, "win_none": {"LM_WFA_WIN": "00000"}}
GROUPS = [g for g in W.GROUPS if g != "long_bounds"]   # (beyond 12 001 bases: the default tuning only)


@pytest.fixture(scope="module")
def index_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("wfa_edges") / "t.lmi")
    O.build_index(d, synth.make_genomes(2, 60000, 1, seed=3, max_div=0.05), O.default_build_opt(chunks=2))
    return d


def align(index_dir, monkeypatch, env, pairs):
    """one wfa() call of a fresh Index opened under env -> results, {kernel name: launches}"""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gi = la.Index(index_dir)
    try:
        gi.profile(True)
        got = gi.wfa([(c.q, c.t) for c in pairs])
        names = {p["name"]: p["launches"] for p in gi.profile_get() if p["name"].startswith("k_wfa") and p["launches"] > 0}
    finally:
        gi.close()
    return got, names


def verify(c, g):
    assert g["status"] in (0, 2), (c.name, g["status"])
    exp = W.expected(c.name)
    assert g["score"] == exp["score"], (c.name, g["score"], exp["score"])
    assert W.same(g, exp), c.name
    W.check_result(c.q, c.t, g)
    if c.longest <= W.DP_MAX:
        dp = W.dp_score(c.name)
        assert g["score"] >= dp, (c.name, g["score"], dp)
        if c.name not in ADAPTIVE_DIFFERS:
            assert g["score"] == dp, (c.name, g["score"], dp)


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_group_under_setting(index_dir, monkeypatch, setting, group):
    pairs = W.by_group(group)
    got, names = align(index_dir, monkeypatch, SETTINGS[setting], pairs)
    print(setting, group, names)
    assert len(got) == len(pairs)
    for c, g in zip(pairs, got):
        verify(c, g)
    if group in ("nonacgt", "outgrow", "many_runs"):   # bytes the packer refuses, wider than every ring, ops overflow
        assert "k_wfa_wide" in names, names
    if group == "outgrow":                             # ... and the widest ring was tried first
        assert "k_wfa_lean1024" in names or "k_wfa_win1024" in names, names
    if group == "window" and setting == "win_all":
        assert any(n.startswith("k_wfa_win") for n in names), names
    if setting == "win_none" and all(c.longest <= 65536 for c in pairs):
        assert not any(n.startswith("k_wfa_win") for n in names), names


@pytest.mark.parametrize("name", [c.name for c in W.by_group("cells16")])
def test_the_limit_of_the_16_bit_cells(index_dir, monkeypatch, name):
    """12 000 / 12 001 bases, each alone in its call and whole in LDS: the pass decides on 16-bit cells from the longest problem
    of its class.  With 32-bit cells everywhere the result must be the same."""
    c = W.by_name(name)
    got16, names16 = align(index_dir, monkeypatch, {"LM_WFA_WIN": "00000"}, [c])
    got32, names32 = align(index_dir, monkeypatch, {"LM_WFA_WIN": "00000", "LM_WFA_R16": "0"}, [c])
    print(name, names16, names32)
    verify(c, got16[0])
    verify(c, got32[0])
    assert got16 == got32
    assert not any(n.startswith("k_wfa_win") for n in list(names16) + list(names32))


@pytest.mark.parametrize("name", [c.name for c in W.by_group("long_bounds")])
def test_long_class_bounds(index_dir, monkeypatch, name):
    """32 768 / 32 769 and 65 536 / 65 537 bases (2048 and 4096 words: the last two class bounds; beyond 65 536 bases only the
    windowed form holds a pair)"""
    c = W.by_name(name)
    got, names = align(index_dir, monkeypatch, {}, [c])
    print(name, names)
    verify(c, got[0])
    if c.longest > 65536:
        assert any(n.startswith("k_wfa_win") for n in names), names
