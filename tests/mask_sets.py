"""Mask sets of the custom-mask tests (test_gpu_build_custom_masks.py, test_mask_plan_cpu.py), all from seeded generators.
A mask is a k-mer as a number: A = 0 .. T = 3, first base in the highest bits; p = max(floor(log4 n), 1) bases of prefix."""
import random


def prefix_bases(n):
    p = 0
    while 4 ** (p + 1) <= n:
        p += 1
    return max(p, 1)


def skewed(k, n, seed=1):
    """the skewed set: every one of the 4^p prefixes gets one mask with random low bits; each remaining mask takes a prefix
    drawn from the lowest eighth of the prefixes (dropped when that prefix already holds 32); sorted and distinct"""
    p = prefix_bases(n)
    npfx, low = 4 ** p, 2 * (k - p)
    rng = random.Random(seed * 1_000_003 + k * 65_536 + n)
    ms = {(f << low) | rng.getrandbits(low) for f in range(npfx)}
    count = [1] * npfx
    for _ in range(n - npfx):
        f = rng.randrange(max(1, npfx // 8))
        m = (f << low) | rng.getrandbits(low)
        if count[f] >= 32 or m in ms:
            continue
        ms.add(m)
        count[f] += 1
    return sorted(ms)


def tall_and_tiny(k, tall=32, seed=7, tall_prefix=5, three_prefix=40):
    """p = 3: prefix `tall_prefix` holds `tall` masks, prefix `three_prefix` 3, each of the other 62 exactly one"""
    low = 2 * (k - 3)
    rng = random.Random(seed * 977 + k)
    ms = set()
    for f in range(64):
        want = tall if f == tall_prefix else 3 if f == three_prefix else 1
        mine = set()
        while len(mine) < want:
            mine.add((f << low) | rng.getrandbits(low))
        ms |= mine
    return sorted(ms)


def per_prefix(k, masks):
    """number of masks on every p-base prefix"""
    p = prefix_bases(len(masks))
    c = [0] * 4 ** p
    for m in masks:
        c[m >> (2 * (k - p))] += 1
    return c
