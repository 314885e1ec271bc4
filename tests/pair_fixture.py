"""The genome sets of the genome-pair tests (test_gpu_genome_pairs.py on the GPU, test_pair_plan_cpu.py for the model's
self-check), about 0.3 Mb each from a seeded random.Random.

P ("pairs"), masks MS.skewed(31, 1500), max_genome = 40 000 (11 records):
  A 40 kb; A2 = A with 2 % substitutions; B 40 kb unrelated; A8 = A with 8 %; Acopy = A exactly; tiny 200 b;
  S = contigs of 30 kb + 25 kb, split into two records; Sx2 = the first contig of S with 1 %; half = A[:20000] + 20 kb random;
  tiny2 = tiny with 1 % + 40 random bases.
C ("clones"), masks MS.skewed(31, 256) (138 records):
  130 identical 3-kb genomes (groups wider than two wavefronts); 6 copies with 3 % substitutions; rep = a 20-kb sequence
  followed by its own 1 % copy (two seeds of one record in a group); rep2 = that sequence with 2 %."""
import random

import mask_sets as MS

K = 31
P_MAX_GENOME = 40_000


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def _mutate(rng, s, frac):
    b = bytearray(s)
    for i in range(len(b)):
        if rng.random() < frac:
            b[i] = rng.choice([c for c in b"ACGT" if c != b[i]])
    return bytes(b)


def p_masks():
    return MS.skewed(K, 1500)


def c_masks():
    return MS.skewed(K, 256)


def p_genomes():
    rng = random.Random(20261020)
    a = _rand(rng, 40_000)
    tiny = _rand(rng, 200)
    s1, s2 = _rand(rng, 30_000), _rand(rng, 25_000)
    gs = [("A", [("A_c", a)]),
          ("A2", [("A2_c", _mutate(rng, a, 0.02))]),
          ("B", [("B_c", _rand(rng, 40_000))]),
          ("A8", [("A8_c", _mutate(rng, a, 0.08))]),
          ("Acopy", [("Acopy_c", a)]),
          ("tiny", [("tiny_c", tiny)]),
          ("S", [("S_1", s1), ("S_2", s2)]),
          ("Sx2", [("Sx2_c", _mutate(rng, s1, 0.01))]),
          ("half", [("half_c", a[:20_000] + _rand(rng, 20_000))]),
          ("tiny2", [("tiny2_c", _mutate(rng, tiny, 0.01) + _rand(rng, 40))])]
    return gs


def p_record_names():
    """genome id of every record of P in record order (S is two records)"""
    out = []
    for gid, contigs in p_genomes():
        out += [gid] * (2 if gid == "S" else 1)
    return out


def c_genomes():
    rng = random.Random(20261021)
    clone = _rand(rng, 3_000)
    gs = [("clone%03d" % i, [("clone%03d_c" % i, clone)]) for i in range(130)]
    gs += [("near%d" % i, [("near%d_c" % i, _mutate(rng, clone, 0.03))]) for i in range(6)]
    r = _rand(rng, 20_000)
    gs.append(("rep", [("rep_c", r + _mutate(rng, r, 0.01))]))
    gs.append(("rep2", [("rep2_c", _mutate(rng, r, 0.02))]))
    return gs
