"""The genome set of the builder tests (test_gpu_build_genomes.py on the GPU, test_build_plan_cpu.py on the host): about
0.7 Mb from a seeded random.Random - 8 input genomes that become 9 genome records (G6 is split at max_genome = 150 000) with
one chunk list of 2.  Every genome is there for something that can break:
  G1 1 x 120 kb                                   baseline
  G2 contigs of 60 kb, 25 b, 1.2 kb, 40 kb        spacers, a contig shorter than k, seq_idx / seq_len
  G3 90 kb with N x 7 at 0, N x 4 at 1000 (no skip region), N x 5 at 2000, N x 300 at 30000, n x 9 at the very end,
     40 lower-case bases, YKR                     skip regions at both ends, the base table
  G4 1 x 6 kb                                     the missing-prefix rule for most masks
  G5 60 kb with A x 2000 and (AC) x 500           deserts whose candidates are low-complexity
  G6 100 kb + 80 kb + 30 kb                       split into 2 records: x, then y + spacer + z
  G7 G1 with 5 % substitutions                    two genomes per query
  G8 1 x 200 b                                    a genome with 170 k-mers
"""
import random

MAX_GENOME = 150_000
K = 31
CONTIG_INTERVAL = 1000


def _rand(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def genomes():
    rng = random.Random(20260117)
    g1 = _rand(rng, 120_000)
    g2 = [("G2_a", _rand(rng, 60_000)), ("G2_b", _rand(rng, 25)), ("G2_c", _rand(rng, 1_200)), ("G2_d", _rand(rng, 40_000))]
    g3 = bytearray(_rand(rng, 90_000))
    g3[0:7] = b"N" * 7
    g3[1000:1004] = b"N" * 4
    g3[2000:2005] = b"N" * 5
    g3[30_000:30_300] = b"N" * 300
    g3[90_000 - 9:] = b"n" * 9
    g3[29_500:29_540] = bytes(g3[29_500:29_540]).lower()
    g3[30_900:30_903] = b"YKR"
    g4 = _rand(rng, 6_000)
    g5 = bytearray(_rand(rng, 60_000))
    g5[10_000:12_000] = b"A" * 2000
    g5[20_000:21_000] = b"AC" * 500
    g6 = [("G6_x", _rand(rng, 100_000)), ("G6_y", _rand(rng, 80_000)), ("G6_z", _rand(rng, 30_000))]
    g7 = bytearray(g1)
    for i in range(len(g7)):
        if rng.random() < 0.05:
            g7[i] = rng.choice([b for b in b"ACGT" if b != g7[i]])
    g8 = _rand(rng, 200)
    return [("G1", [("G1_c", g1)]), ("G2", g2), ("G3", [("G3_c", bytes(g3))]), ("G4", [("G4_c", g4)]),
            ("G5", [("G5_c", bytes(g5))]), ("G6", g6), ("G7", [("G7_c", bytes(g7))]), ("G8", [("G8_c", g8)])]


def queries(gs):
    """the six queries (every one returns rows): G1[50000:51500] (two genomes: G1 and G7); G3[29000:31500] upper-cased (across
    the 300 N); contig y of G6 [1000:3000] (record 6 = chunk 1 of 2); G4[1000:2500]; contig d of G2 [100:1600] (seq_idx 3);
    G5[9500:12500] (across the A run)"""
    d = dict(gs)
    return [d["G1"][0][1][50_000:51_500], d["G3"][0][1][29_000:31_500].upper(), d["G6"][1][1][1_000:3_000],
            d["G4"][0][1][1_000:2_500], d["G2"][3][1][100:1_600], d["G5"][0][1][9_500:12_500]]


def concatenation(contigs, interval=CONTIG_INTERVAL):
    """the bases a genome record stores for these contigs: spacers of A, the 2-bit table of genome/genome.go:1427-1444 and back"""
    tab = bytearray(b"A" * 256)
    for src, dst in ((b"Aa", b"A"), (b"CcBbSsYy", b"C"), (b"GgKk", b"G"), (b"TtUu", b"T")):
        for c in src:
            tab[c] = dst[0]
    return (b"A" * interval).join(bytes(s).translate(bytes(tab)) for _, s in contigs)


def records(gs, max_genome=MAX_GENOME, interval=CONTIG_INTERVAL):
    """(genome id, contigs) of every genome record, in record order: the split of lib-index-build.go:1581-1658 restated"""
    out = []
    for gid, contigs in gs:
        cur, first = 0, 0
        for i, (_, s) in enumerate(contigs):
            if cur + len(s) > max_genome and i > first:
                out.append((gid, contigs[first:i]))
                first, cur = i, 0
            if i > first:
                cur += interval
            cur += len(s)
        out.append((gid, contigs[first:]))
    return out
