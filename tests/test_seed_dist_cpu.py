"""lm_index_seed_positions / lm_index_seed_distances without a GPU: the distance rule of lm_seed_dist.h, built for the host
into a stand-alone program under AddressSanitizer and UBSan and checked against a plain loop (tests/seed_dist_host.cpp); the
declarations, the exported symbols and the Python view."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "lexicmap_amd", "csrc")

NEW_SYMBOLS = ("lm_index_seed_positions", "lm_seedpos_free", "lm_index_seed_distances", "lm_seed_dist_free",
               "lm_seedpos_get", "lm_seed_dist_records", "lm_seed_dist_hist", "lm_seed_dist_rows")


def test_distance_rule_equals_a_plain_loop_under_sanitizers(tmp_path):
    exe = str(tmp_path / "seed_dist_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "seed_dist_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    for case in ("position at a contig start, last k-mer of a contig", "seedless contig in the middle", "duplicates", "single contig",
                 "empty list", "only the last contig", "interval 0"):
        assert "ok " + case in lines, r.stdout
    assert "FAIL" not in r.stdout and not r.stderr


def test_the_rule_header_has_no_hip_types():
    txt = open(os.path.join(CSRC, "lm_seed_dist.h")).read()
    code = re.sub(r"//.*", "", txt)
    assert "hip/" not in code and "threadIdx" not in code and "__global__" not in code
    # the kernel file compiles the same header
    assert '#include "lm_seed_dist.h"' in open(os.path.join(CSRC, "lm_seedpack.hip")).read()


def test_new_symbols_are_declared_and_exported_and_the_header_is_c99():
    import lexicmap_amd as la
    la.build_library()
    hdr = os.path.join(ROOT, "include", "lexicmap_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    assert re.search(r"lm_status\s+lm_index_seed_positions\s*\(\s*lm_index\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*lm_seedpos\s*\*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"lm_status\s+lm_index_seed_distances\s*\(\s*lm_index\s*\*\s*\w+\s*,\s*const\s+uint64_t\s*\*\s*\w+\s*,\s*size_t\s+\w+\s*,"
                     r"\s*const\s+lm_seed_dist_opt\s*\*\s*\w+\s*,\s*lm_seed_dist\s*\*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"void\s+lm_seedpos_free\s*\(\s*lm_seedpos\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"void\s+lm_seed_dist_free\s*\(\s*lm_seed_dist\s*\*\s*\w+\s*\)\s*;", txt)
    out = subprocess.check_output(["nm", "-D", "--defined-only", la.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for f in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % f, txt), f
        assert f in exported, f
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_python_view_matches_the_c_structs(tmp_path):
    """the ctypes structures against sizeof / offsetof of the header's, through a small C program"""
    import ctypes as C
    import lexicmap_amd as la
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lexicmap_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(lm_seed_dist_opt), sizeof(lm_seed_dist_rec), sizeof(lm_seed_dist_row),'
                   ' offsetof(lm_seed_dist_rec, max_dist_pos), offsetof(lm_seed_dist_rec, contigs_without_seeds), offsetof(lm_seed_dist_row, dist)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.check_output([exe]).split()]
    A = la.api
    assert got == [C.sizeof(A.SeedDistOpt), C.sizeof(A.SeedDistRec), C.sizeof(A.SeedDistRow), A.SeedDistRec.max_dist_pos.offset,
                   A.SeedDistRec.contigs_without_seeds.offset, A.SeedDistRow.dist.offset]
    assert hasattr(la.Index, "seed_positions") and hasattr(la.Index, "seed_distances")
