"""-a/--all with a sharded index: the cigar / qseq / sseq / align columns travel through the row gather and follow their rows
through the device merge (lm_gather_rows_ex / lm_gather_merge_rows_ex / lm_merge_sharded_device_ex with LM_ROW_ALL,
lexicmap_amd/csrc/lm_comm.cpp + lm_merge.hip).  Two PROCESSES on the one GPU, each with its own communicator rank; the nine
nccl* symbols come from tests/fake_rccl.c (Unix sockets + hipMemcpy) through LM_RCCL_LIB, as in test_gpu_gather_two_procs.py.

1. two genome shards of an index opened with output_seq=1, gathered to root 0 and to root 1: the device merge and the host
   gather + lm_merge_sharded_ex give the unsharded handle's rows - every column, the names and the four strings; flags 0 in the
   same workers still give NULL strings;
2. -a -n 2 from two shards (one demo genome each) prints the reference's golden TSV byte for byte;
3. one process: the device merge of four synthetic shards in the wire form (blocks of 16 B to 1 MB, NULL and empty strings, an
   empty shard) equals the host merge of the same rows, byte for byte."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "demo")

WORKER = r'''
import os, pickle, sys, time
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(here)r)
import numpy as np
import lexicmap_amd as la
from lexicmap_amd import merge
from lexicmap_amd.api import Comm, row_names, row_strings
rank, d, tmp, mode = int(sys.argv[1]), sys.argv[2], sys.argv[3], sys.argv[4]


def publish(name, obj):
    p = os.path.join(tmp, name)
    pickle.dump(obj, open(p + ".tmp", "wb"))
    os.rename(p + ".tmp", p)


def fetch(name):
    p = os.path.join(tmp, name)
    for _ in range(6000):
        if os.path.exists(p):
            return pickle.load(open(p, "rb"))
        time.sleep(0.02)
    raise RuntimeError("no " + name)


if rank == 0:
    publish("id.bin", Comm.unique_id())
comm = Comm(fetch("id.bin"), 2, rank, device=0)
meta = pickle.load(open(os.path.join(tmp, "meta.pkl"), "rb"))
strs = lambda a: [row_strings(a, i) for i in range(len(a))]
names = lambda a: [row_names(a, i) for i in range(len(a))]
out = {}
if mode == "rows":
    gi = la.Index(d, la.api.default_options(shard_count=2, shard_rank=rank, output_seq=1, total_bases_override=meta["tb"]))
    qb = gi.upload([q[1] for q in meta["queries"]])
    rows, _ = gi.search_resident_np(qb)   # a view: its strings stay live while `rows` is (no .copy() of the rows)
    out["own"] = len(rows)
    out["own_strs"] = strs(rows)
    for root in (0, 1):
        m = comm.gather_merge_rows(rows, root=root, index=gi, strings=True)
        if rank == root:
            out["dev_%%d" %% root] = (m.copy(), strs(m), names(m))
        per_rank, counts = comm.gather_rows(rows, root=root, strings=True)
        if rank == root:
            out["gat_%%d" %% root] = [strs(p) for p in per_rank]
            h = merge.merge_sharded_c(per_rank, index=gi, strings=True)
            out["host_%%d" %% root] = (h.copy(), strs(h), names(h))
        m0 = comm.gather_merge_rows(rows, root=root, index=gi)        # flags 0: the plain calls
        if rank == root:
            out["dev0_%%d" %% root] = m0.copy()
        p0, _ = comm.gather_rows(rows, root=root)
        if rank == root:
            out["gat0_%%d" %% root] = merge._cat(p0)
    del rows
else:  # "golden": -a -n 2 over two shards
    qs = meta["queries"]
    gi = la.Index(d, la.api.default_options(shard_count=2, shard_rank=rank, output_seq=1, top_n_genomes=2, total_bases_override=meta["tb"]))
    qb = gi.upload([q[1] for q in qs])
    publish("cand%%d.pkl" %% rank, gi.search_scores(qb))
    kq, kg = merge.topn_merge([fetch("cand0.pkl"), fetch("cand1.pkl")], 2)
    rows, _ = gi.search_resident_keep_np(qb, kq, kg)
    out["own"] = len(rows)
    m = comm.gather_merge_rows(rows, root=0, index=gi, strings=True)
    if rank == 0:
        text, _ = la.api.format_rows(m, [q[0] for q in qs], [len(q[1]) for q in qs], flags=la.api.LM_ROW_ALL)
        out["tsv"] = la.lib().lm_tsv_header(1) + b"\n" + text
    del rows
comm.close()
gi.close()
publish("out%%d.pkl" %% rank, out)
'''

DEVICE_WORKER = r'''
import ctypes as C, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch
from lexicmap_amd import merge
from lexicmap_amd.api import Comm, row_strings

rng = np.random.default_rng(23)
COUNTS = [700, 0, 900, 500]
ALPH = np.frombuffer(b"ACGTacgtMIDX=|. -", dtype=np.uint8)


def rnd(n):
    return ALPH[rng.integers(0, len(ALPH), n)].tobytes()


def strings(uid):
    if uid %% 13 == 5:
        return (None, None, None, None)
    if uid == 40:   # a block of 1 MB and a bit: 17 chunks of 64 KB
        return (b"300M", rnd(349_000), rnd(349_000), rnd(350_000))
    if uid == 41:   # exactly one 64-KB chunk
        return (rnd(65_535), None, None, None)
    if uid == 1500: # one byte over a chunk
        return (rnd(65_536), None, None, None)
    if uid == 1501: # a 4-byte block before padding
        return (b"", b"", b"", b"")
    out = []
    for k in range(4):
        r = (uid * 5 + k) %% 7
        out.append(None if r == 0 else b"" if r == 1 else rnd(int(rng.integers(1, 3000))))
    return tuple(out)


shards, allstr, keep = [], [], []
uid = 0
for r, n in enumerate(COUNTS):
    a = np.zeros(n, dtype=merge.ROW_DTYPE)
    qs = np.sort(rng.integers(0, 30, n))
    gs = rng.integers(0, 20, n) * len(COUNTS) + r
    o = np.lexsort((gs, qs))
    a["query"], a["batch_genome"] = qs[o], gs[o]
    a["bitscore"] = rng.choice([100, 250, 400], n)
    a["pident"] = rng.choice([95.0, 100.0], n)
    a["matched_bases"] = np.arange(uid, uid + n)
    for i in range(n):
        allstr.append(strings(uid))
        uid += 1
    shards.append(a)
rows = merge._cat(shards)
total = len(rows)
lens, blob = merge.pack_strings(allstr)
assert max(merge.pack_strings([s])[1].__len__() for s in allstr) > 1_000_000

# the device side: rows, then lengths + blocks in the documented wire form
d_rows = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
wire = np.frombuffer(lens.tobytes() + blob, dtype=np.uint8).copy()
d_str = torch.from_numpy(wire).cuda()
assert d_str.data_ptr() %% 16 == 0
comm = Comm(Comm.unique_id(), 1, 0, device=0)

# the host side: the same rows with live string pointers
hshards, o = [], 0
for a in shards:
    h = a.copy()
    for i in range(len(h)):
        for f, x in zip(("cigar", "qseq", "sseq", "align"), allstr[o + i]):
            if x is not None:
                b = C.create_string_buffer(x)
                keep.append(b)
                h[f][i] = C.addressof(b)
    o += len(a)
    hshards.append(h)
host = merge.merge_sharded_c(hshards, strings=True)
host_strs = [row_strings(host, i) for i in range(total)]
cols = lambda a: [(f, np.ascontiguousarray(a[f]).tobytes()) for f in merge.ROW_DTYPE.names if f not in merge.PTR_FIELDS]

for rep in range(2):   # (the second call reuses the grow-only buffers)
    dev = comm.merge_sharded_device(d_rows.data_ptr(), COUNTS, strings_ptr=d_str.data_ptr(), string_bytes=len(blob))
    assert len(dev) == total
    assert cols(dev) == cols(host), rep
    for i in range(total):
        assert row_strings(dev, i) == host_strs[i], (rep, i)
    for f in ("genome_id", "seq_id"):
        assert (dev[f] == 0).all()
plain = comm.merge_sharded_device(d_rows.data_ptr(), COUNTS)
assert cols(plain) == cols(host) and all((plain[f] == 0).all() for f in merge.PTR_FIELDS)
try:    # lengths that do not add up to the bytes: refused before anything is copied
    comm.merge_sharded_device(d_rows.data_ptr(), COUNTS, strings_ptr=d_str.data_ptr(), string_bytes=len(blob) - 16)
    raise AssertionError("a wrong string_bytes was accepted")
except RuntimeError as e:
    assert "(7)" in str(e), e
dev = comm.merge_sharded_device(d_rows.data_ptr(), COUNTS, strings_ptr=d_str.data_ptr(), string_bytes=len(blob))
assert [row_strings(dev, i) for i in range(total)] == host_strs
comm.close()
print("device merge of %%d rows, %%d string bytes = the host merge" %% (total, len(blob)))
'''


@pytest.fixture(scope="module")
def fake_rccl(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fake") / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O2", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(HERE, "fake_rccl.c"), "-o", so,
                           "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"])
    return so


def _run(cmds, env, timeout=600):
    """start every command, wait for all under a time limit; the first nonzero exit fails the test (the others are killed)"""
    procs = [subprocess.Popen(c, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for c in cmds]
    outs = []
    try:
        for p in procs:
            so, se = p.communicate(timeout=timeout)
            if p.returncode != 0:
                raise AssertionError("exit %d:\n%s\n%s" % (p.returncode, so[-2000:], se[-4000:]))
            outs.append(so)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return outs


def _two_ranks(tmp_path, fake_rccl, d, mode, meta):
    pickle.dump(meta, open(str(tmp_path / "meta.pkl"), "wb"))
    script = str(tmp_path / "worker.py")
    open(script, "w").write(WORKER % dict(root=ROOT, here=HERE))
    env = dict(os.environ, LM_RCCL_LIB=fake_rccl, LM_FAKE_RCCL_DIR=str(tmp_path))
    _run([[sys.executable, script, str(r), d, str(tmp_path), mode] for r in (0, 1)], env)
    return [pickle.load(open(str(tmp_path / ("out%d.pkl" % r)), "rb")) for r in (0, 1)]


def _cols(a):
    from lexicmap_amd import merge
    return [(f, np.ascontiguousarray(a[f]).tobytes()) for f in merge.ROW_DTYPE.names if f not in merge.PTR_FIELDS]


def test_strings_travel_through_the_gather_and_both_merges(tmp_path, fake_rccl):
    import lexicmap_amd as la
    from lexicmap_amd import merge, synth
    genomes = synth.make_genomes(12, 70_000, 3, seed=5, max_div=0.06, contigs=(1, 2))
    queries = synth.make_gene_queries(genomes, 20, seed=6, len_range=(500, 1600), max_div=0.08)
    d = str(tmp_path / "two.lmi")
    O.build_index(d, genomes, O.default_build_opt(chunks=2))
    gi = la.Index(d, la.api.default_options(output_seq=1))
    tb = gi.info()["total_bases"]
    ref, _ = gi.search_resident_np(gi.upload([q[1] for q in queries]))
    ref_strs = [la.api.row_strings(ref, i) for i in range(len(ref))]
    ref_names = [la.api.row_names(ref, i) for i in range(len(ref))]
    ref = ref.copy()
    gi.close()
    assert len(ref) > 40 and any(s[1] for s in ref_strs)
    outs = _two_ranks(tmp_path, fake_rccl, d, "rows", dict(queries=queries, tb=tb))
    assert outs[0]["own"] > 0 and outs[1]["own"] > 0 and outs[0]["own"] + outs[1]["own"] == len(ref)
    for root in (0, 1):
        got = outs[root]
        for kind in ("dev", "host"):   # lm_gather_merge_rows_ex / lm_gather_rows_ex + lm_merge_sharded_ex
            rows, s, nm = got["%s_%d" % (kind, root)]
            assert _cols(rows) == _cols(ref), kind
            assert nm == ref_names, kind
            assert s == ref_strs, kind
        assert got["gat_%d" % root] == [outs[0]["own_strs"], outs[1]["own_strs"]]   # the gathered rows carry their own strings
        for plain in (got["dev0_%d" % root], got["gat0_%d" % root]):           # flags 0: unchanged, NULL strings
            for f in ("cigar", "qseq", "sseq", "align"):
                assert (plain[f] == 0).all()
        assert _cols(got["dev0_%d" % root]) == _cols(ref)
        assert "dev_%d" % root not in outs[1 - root]


def test_all_columns_top_n_from_two_shards_print_the_reference_golden(tmp_path, fake_rccl):
    import lexicmap_amd as la
    d = str(tmp_path / "demo2.lmi")
    genomes = [(f[:-6], O.read_fasta(os.path.join(GOLD, f))) for f in ("GCF_002949675.1.fa.gz", "GCF_003697165.2.fa.gz")]
    O.build_index(d, genomes, O.default_build_opt(chunks=4))
    gi = la.Index(d)
    tb = gi.info()["total_bases"]
    gi.close()
    qs = [(q[0].decode() if isinstance(q[0], bytes) else q[0], q[1]) for q in O.read_fasta(os.path.join(GOLD, "q.gene.fasta"))]
    outs = _two_ranks(tmp_path, fake_rccl, d, "golden", dict(queries=qs, tb=tb))
    assert outs[0]["own"] > 0 and outs[1]["own"] > 0          # each shard holds one of the two genomes
    gold = open(os.path.join(GOLD, "q.gene.fasta.lexicmap_top-2-genomes_all.tsv"), "rb").read()
    assert outs[0]["tsv"] == gold
    assert "tsv" not in outs[1]


def test_device_merge_of_the_wire_form_equals_the_host_merge(tmp_path, fake_rccl):
    script = str(tmp_path / "device_worker.py")
    open(script, "w").write(DEVICE_WORKER % dict(root=ROOT))
    env = dict(os.environ, LM_RCCL_LIB=fake_rccl, LM_FAKE_RCCL_DIR=str(tmp_path))
    out = _run([[sys.executable, script]], env)[0]
    assert "= the host merge" in out
