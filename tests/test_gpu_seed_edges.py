"""GPU: seed lookup and seed chaining (k_lookup_prep / _count / _emit / _emit_flat, k_chain1, k_chain1_wave) on indexes of tiny
genomes, where every lookup can end in a flat outlier list and where the reference's anchor index hides runs of k-mers from
its own search.  One lm_seed_chain_batch per index and variant over the whole case batch of seed_cases.py, compared with

  the oracle       same (query, genome) pairs; raw anchors in ClearSubstrPairs order, cleared anchors, score bits, chains
  the plain model  (seed_model.py) the raw anchors of every pair as a multiset

test_seed_edges_cpu.py asserts, without a GPU, that these cases reach the edges they were made for (outlier lookups, lookups
lost to the start rule, 65 values and more, several query locations, pair sizes around 48 / 64 / 128, ...).

Variants: the defaults; LM_LOOKUP_FLAT=0 (k_lookup_emit); LM_CHAIN1_WAVE=0 (every pair by a lane of k_chain1); -p at its lower
bound; -p = -P = k; and on V2k three genome whitelists (k_lookup_emit and the kept-count loops of k_lookup_count).
"""
import ctypes as C

import numpy as np
import pytest

import seed_cases as SC
import seed_model as SM

pytestmark = pytest.mark.gpu

VARIANTS = {  # name -> (option set, environment, whitelist)
    "default": ("default", {}, None),
    "flat0": ("default", {"LM_LOOKUP_FLAT": "0"}, None),
    "wave0": ("default", {"LM_CHAIN1_WAVE": "0"}, None),
    "p_lo": ("p_lo", {}, None),
    "p_k": ("p_k", {}, None),
}
WHITELISTS = {
    "keep_tiny": lambda n: list(range(1, n)),
    "keep_big": lambda n: [0],
    "keep_every_second": lambda n: list(range(0, n, 2)),
}
PARAMS = [(n, v) for n in SC.INDEXES for v in VARIANTS] + [("V2k", w) for w in WHITELISTS]


def _la():
    import lexicmap_amd as la
    return la


_cases = {}


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("seed_edges_gpu"))

    def get(name):
        if name not in _cases:
            _cases[name] = SC.Case(name, d)
        return _cases[name]
    yield get
    _cases.clear()


def _dtype(struct):
    names = [f[0] for f in struct._fields_]
    return np.dtype(dict(names=names, formats=[np.dtype(f[1]) for f in struct._fields_],
                         offsets=[getattr(struct, n).offset for n in names], itemsize=C.sizeof(struct)))


def _view(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(C.addressof(ptr.contents)), dtype=dtype).copy()


def seed_chain(gi, seqs):
    """lm_seed_chain_batch read through numpy views (Index.seed_chain builds a tuple per anchor: too slow for the 40 000-anchor
    pairs here): {(query, genome): (raw rows, cleared rows, score, chains)}"""
    api = _la().api
    L = api.lib()
    arr, keep = api._queries(seqs)
    sg, npairs = C.c_void_p(), C.c_size_t()
    pairs, raw, clr = C.POINTER(api.Pair)(), C.POINTER(api.Anchor)(), C.POINTER(api.Anchor)()
    cptr, cidx = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)()
    st = L.lm_seed_chain_batch(gi.h, arr, len(seqs), C.byref(sg), C.byref(npairs), C.byref(pairs), C.byref(raw), C.byref(clr),
                               C.byref(cptr), C.byref(cidx))
    if st != 0:
        gi._err(st)
    P = _view(pairs, npairs.value, _dtype(api.Pair))
    nraw = int((P["raw_off"] + P["raw_n"]).max()) if len(P) else 0
    nclr = int((P["clr_off"] + P["clr_n"]).max()) if len(P) else 0
    nch = int((P["chain_off"] + P["chain_n"]).max()) if len(P) else 0
    R, Cl = SC.rows(_view(raw, nraw, SC.SUB_DTYPE)), SC.rows(_view(clr, nclr, SC.SUB_DTYPE))
    cp = np.ctypeslib.as_array(cptr, shape=(nch + 1,)).copy()
    ci = np.ctypeslib.as_array(cidx, shape=(max(int(cp[nch]), 1),)).copy()
    L.lm_stage_free(sg)
    out = {}
    for p in P:
        ro, rn, co, cn, ho, hn = (int(p[f]) for f in ("raw_off", "raw_n", "clr_off", "clr_n", "chain_off", "chain_n"))
        chains = [ci[cp[ho + x]:cp[ho + x + 1]].tolist() for x in range(hn)]
        key = (int(p["query"]), int(p["batch_genome"]))
        assert key not in out
        out[key] = (R[ro:ro + rn], Cl[co:co + cn], np.float32(p["score"]), chains)
    return out


@pytest.mark.parametrize("name,variant", PARAMS)
def test_seed_lookup_and_chaining_on_tiny_genome_indexes(case, monkeypatch, name, variant):
    la = _la()
    c = case(name)
    keep = None
    if variant in WHITELISTS:
        oname, env, keep = "default", {}, WHITELISTS[variant](len(c.genomes))
    else:
        oname, env, _ = VARIANTS[variant]
    s = c.set(oname)
    exp = c.chained(oname)
    model = s["model"] if keep is None else c.model_kept(oname, keep)
    for k, v in env.items():
        monkeypatch.setenv(k, v)   # (read once, when the handle is created)
    gi = la.Index(c.dir, la.api.default_options(**s["kw"]))
    try:
        info = gi.info()
        assert info["outlier_seeds"] > 0 and info["anchor_prefix"] == c.lists.a and info["mask_prefix"] == c.lists.p
        if keep is not None:
            gi.set_genome_filter([SC.genome_key(i) for i in keep])
        got = seed_chain(gi, c.seqs)
        stats = None
        if variant == "default":
            _rows, stats = gi.search(c.seqs)
    finally:
        gi.close()
    kept = None if keep is None else {SC.genome_key(i) for i in keep}
    want = {(qi, g): v for qi, per in enumerate(exp) for g, v in per.items() if kept is None or g in kept}
    n_gpu, n_exp = sum(len(v[0]) for v in got.values()), sum(len(v[0]) for v in want.values())
    print("%s %s: pairs gpu %d oracle %d, raw anchors gpu %d oracle %d" % (name, variant, len(got), len(want), n_gpu, n_exp))
    assert n_exp > 1000 and len(want) >= 5
    extra, missing = sorted(set(got) - set(want)), sorted(set(want) - set(got))
    assert not extra and not missing, (len(extra), len(missing), [(c.names[q], g) for q, g in (extra + missing)[:6]])
    assert {(qi, g) for qi, per in enumerate(model) for g in per} == set(want)
    for (qi, g), (raw, cleared, score, chains) in want.items():
        graw, gclr, gscore, gchains = got[(qi, g)]
        label = (c.names[qi], g, len(raw), len(graw))
        assert np.array_equal(graw, raw), label
        assert np.array_equal(SM.sorted_rows(graw), model[qi][g]), label
        assert np.array_equal(gclr, cleared), label
        assert np.float32(gscore).tobytes() == np.float32(score).tobytes(), label
        assert gchains == chains, label
    if keep is not None:
        assert sum(len(r) for per in model for r in per.values()) == n_exp
    if stats is not None:  # the whole search ran the same lookups
        assert stats["seed_lookups"] > 0 and stats["genome_pairs"] == len(want)
        assert stats["anchors_raw"] == n_exp
