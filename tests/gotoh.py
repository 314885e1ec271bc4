"""ctypes binding of tests/libgotoh_host.so (tests/gotoh_host.cpp): the exact gap-affine global alignment score by plain
three-matrix dynamic programming.  The WFA tests hold the oracle, the host-compiled device code and the kernels to it; it shares
no code with any of them.  Test infrastructure only."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gotoh_host.cpp")
LIB = os.path.join(HERE, "libgotoh_host.so")

MISMATCH, GAP_OPEN, GAP_EXTEND = 4, 6, 2   # the reference's wfa.DefaultPenalties

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
            subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC])
        L = C.CDLL(LIB)
        L.gotoh_score.restype = C.c_int32
        L.gotoh_score.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        _lib = L
    return _lib


def score(q, t):
    """the least cost of a global alignment of the byte strings q and t: mismatch 4, a gap of n bases 6 + 2 n"""
    return lib().gotoh_score(q, len(q), t, len(t), MISMATCH, GAP_OPEN, GAP_EXTEND)
