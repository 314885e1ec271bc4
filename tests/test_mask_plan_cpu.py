"""The mask-set rule of the index builder (lexicmap_amd/csrc/lm_mask_plan.h: validation, prefix CSR, fullest prefix,
once-or-twice) without a GPU: built for the host into a stand-alone program under AddressSanitizer and UBSan
(tests/mask_plan_host.cpp), run on the mask sets of the GPU tests and on every refusal, against expectations computed here.
Then the new declaration: exported, the header still C99, and the refusals through the C-ABI, which need no device."""
import os
import re
import subprocess

import pytest

import mask_sets as MS

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "lexicmap_amd", "csrc")


def _expect(k, masks):
    """what plan_masks must say: ("ok", p, max, once_or_twice, pfx_first) or ("refused", the number the text must name)"""
    n = len(masks)
    if not 10 <= k <= 32:
        return ("refused", str(k))
    if not 4 <= n <= 65535:
        return ("refused", str(n))
    for i, m in enumerate(masks):
        if m >= 4 ** k or (i and m <= masks[i - 1]):
            return ("refused", "mask %d " % i)
    c = MS.per_prefix(k, masks)
    for f, x in enumerate(c):
        if x < 1:
            return ("refused", "prefix %d " % f)
        if x > 32:
            return ("refused", "prefix %d has %d masks" % (f, x))
    first = [0]
    for x in c:
        first.append(first[-1] + x)
    return ("ok", MS.prefix_bases(n), max(c), int(max(c) <= 2), first)


def _generated_like(k, n, seed):
    """every prefix once, n - 4^p of them twice: the shape of a generated set"""
    import random
    p = MS.prefix_bases(n)
    low = 2 * (k - p)
    rng = random.Random(seed)
    ms = set()
    for f in range(4 ** p):
        ms.add((f << low) | rng.getrandbits(low - 1))
    for f in rng.sample(range(4 ** p), n - 4 ** p):
        ms.add((f << low) | (1 << (low - 1)) | rng.getrandbits(low - 1))
    return sorted(ms)


def _cases():
    c = {}
    for k, n in ((31, 500), (21, 24), (32, 500), (27, 2048), (31, 20_000), (31, 24_000), (31, 40_000)):
        c["skewed_%d_%d" % (k, n)] = (k, MS.skewed(k, n))
    for k in (31, 12, 10, 32):
        c["tall_%d" % k] = (k, MS.tall_and_tiny(k))
        c["tall33_%d" % k] = (k, MS.tall_and_tiny(k, tall=33))                  # refused: 33 on prefix 5
    c["once_or_twice_31_1500"] = (31, _generated_like(31, 1500, 1))
    c["once_or_twice_31_20000"] = (31, _generated_like(31, 20_000, 2))          # p = 7
    c["once_or_twice_10_7"] = (10, _generated_like(10, 7, 3))                   # p = 1
    c["once_or_twice_32_24"] = (32, _generated_like(32, 24, 4))                 # p = 2
    c["p1_k32_top"] = (32, [0, 1 << 62, 2 << 62, 3 << 62, 2 ** 64 - 1])         # the largest mask there is
    good = MS.skewed(31, 500)
    c["not_ascending"] = (31, good[:100] + [good[100], good[99]] + good[102:])  # mask 101 is the first offender
    c["duplicate"] = (31, good[:7] + [good[6]] + good[8:])                      # mask 7
    c["too_large"] = (21, MS.skewed(21, 24)[:-1] + [4 ** 21])                   # mask 23
    c["too_large_k10"] = (10, [0, 1 << 18, 2 << 18, 3 << 18, 1 << 20])          # mask 4
    c["empty_prefix"] = (31, [m for m in good if m >> 54 != 200])               # prefix 200 of 256
    c["empty_last_prefix"] = (31, [m for m in good if m >> 54 != 255])
    c["k9"] = (9, [0, 1 << 16, 2 << 16, 3 << 16])
    c["k33"] = (33, [0, 1 << 62, 2 << 62, 3 << 62])
    c["n3"] = (31, [0, 1 << 60, 2 << 60])
    c["n65536"] = (31, list(range(0, 65536 << 40, 1 << 40)))
    c["n_near_65535"] = (31, MS.skewed(31, 65535, seed=3))                      # (what the generator kept of 65535: p = 7 either way)
    return c


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("maskplan")
    exe = str(d / "mask_plan_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "mask_plan_host.cpp")])
    cases = _cases()
    inp = d / "cases.txt"
    with open(inp, "w") as f:
        for name, (k, ms) in cases.items():
            f.write("case %s %d %d\n%s\n" % (name, k, len(ms), " ".join("%x" % m for m in ms)))
        for n in (1, 4, 15, 16, 63, 64, 97, 16383, 16384, 65535, 65536):
            f.write("prefix %d\n" % n)
    r = subprocess.run([exe, str(inp)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = {}
    for line in r.stdout.splitlines():
        w = line.split(" ", 2)
        out[w[0] if w[0] != "prefix" else "prefix %s" % w[1]] = (w[1], w[2]) if w[0] != "prefix" else w[2]
    return cases, out


def test_every_case_equals_the_expectation_computed_here(run):
    cases, out = run
    seen = {"ok": 0, "refused": 0}
    for name, (k, ms) in cases.items():
        exp = _expect(k, ms)
        verdict, rest = out[name]
        assert verdict == exp[0], (name, verdict, rest[:200])
        seen[verdict] += 1
        if verdict == "refused":
            assert exp[1] in rest + " ", (name, exp[1], rest)
        else:
            got = [int(x) for x in rest.split()]
            assert got[:3] == list(exp[1:4]), (name, got[:3], exp[1:4])
            assert got[3:] == exp[4], name
    assert seen["ok"] >= 15 and seen["refused"] >= 12


def test_the_cases_cover_what_they_are_meant_to(run):
    cases, out = run
    ok = {n: [int(x) for x in out[n][1].split()[:3]] for n in cases if out[n][0] == "ok"}
    assert {v[0] for v in ok.values()} >= {1, 2, 3, 4, 5, 7}                    # p (8 needs 65536 masks: refused by the count)
    assert {cases[n][0] for n in ok} >= {10, 12, 21, 27, 31, 32}                # k
    for n in ("skewed_31_500", "skewed_21_24", "skewed_32_500", "skewed_27_2048", "skewed_31_20000", "skewed_31_24000", "skewed_31_40000"):
        assert ok[n][1] >= 3 and ok[n][2] == 0, (n, ok[n])                      # three or more on the fullest prefix: CSR
    assert 12 < ok["skewed_31_40000"][1] <= 32                                  # (23 616 extra masks on 2048 prefixes: 12.5 each on average)
    for n in ("tall_31", "tall_12", "tall_10", "tall_32"):
        assert ok[n] == [3, 32, 0] and len(cases[n][1]) == 97
    for n in ("once_or_twice_31_1500", "once_or_twice_31_20000", "once_or_twice_10_7", "once_or_twice_32_24"):
        assert ok[n][1:] == [2, 1], (n, ok[n])                                  # the unchanged instantiation
    assert ok["p1_k32_top"] == [1, 2, 1]
    assert "prefix 5 has 33 masks" in out["tall33_31"][1] and "prefix 5 has 33 masks" in out["tall33_10"][1]
    assert "mask 101 " in out["not_ascending"][1] and "mask 7 equals mask 6" in out["duplicate"][1]
    assert "mask 23 " in out["too_large"][1] and "mask 4 " in out["too_large_k10"][1]
    assert "prefix 200 " in out["empty_prefix"][1] and "prefix 255 " in out["empty_last_prefix"][1]
    assert [out["prefix %d" % n] for n in (1, 4, 15, 16, 63, 64, 97, 16383, 16384, 65535, 65536)] == \
        ["1", "1", "1", "2", "2", "3", "3", "6", "7", "7", "8"]


def test_the_rule_header_has_no_hip_types():
    txt = open(os.path.join(CSRC, "lm_mask_plan.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "hip/" not in code and "__device__" not in code and "__global__" not in code and "lm_internal" not in code
    assert '#include "lm_mask_plan.h"' in open(os.path.join(CSRC, "lm_builder.hip")).read()


def test_new_masks_is_declared_exported_and_refuses_without_a_device():
    """lm_index_builder_new_masks checks the set before it asks for a device: the refusals and their texts here, the builds on
    the GPU (test_gpu_build_custom_masks.py)"""
    import lexicmap_amd as la
    la.build_library()
    hdr = os.path.join(ROOT, "include", "lexicmap_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert re.search(r"lm_status\s+lm_index_builder_new_masks\s*\(\s*const\s+lm_build_opt\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+lm_options\s*\*\s*\w+\s*,\s*const\s+lm_residency\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*lm_index_builder\s*\*\*\s*\w+\s*\)\s*;", txt)
    out = subprocess.check_output(["nm", "-D", "--defined-only", la.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    declared = set(re.findall(r"\b(lm_[a-z0-9_]+)\s*\(", txt))
    assert "lm_index_builder_new_masks" in exported and not [s for s in declared if s not in exported]
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for k, ms, word in ((31, MS.tall_and_tiny(31, tall=33), "prefix 5 has 33 masks"), (9, [0, 1 << 16, 2 << 16, 3 << 16], "k = 9"),
                        (33, [0, 1, 2, 3], "k = 33"), (31, [0, 1 << 60, 2 << 60], "3 masks"),
                        (31, [0, 1 << 60, 1 << 60, 3 << 60], "mask 2 equals mask 1"), (21, [0, 1 << 40, 2 << 40, 4 ** 21], "mask 3 "),
                        (31, [0, 1 << 60, 3 << 60, (3 << 60) + 1], "prefix 2 ")):
        with pytest.raises(ValueError) as ei:
            la.IndexBuilder(la.BuildOpt.default(k=k), masks=ms)
        assert ei.value.status == 7 and word in str(ei.value) and "lm_index_builder_new_masks" in str(ei.value), (word, str(ei.value))
    assert hasattr(la.Index, "masks") and hasattr(la, "read_mask_file") and hasattr(la, "write_mask_file")
