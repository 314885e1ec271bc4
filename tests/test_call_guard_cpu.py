"""The call guard of the resident-index entry points (lm::guarded, lexicmap_amd/csrc/lm_internal.h; the mapping is the table
in INTEGRATION.md) without a GPU: tests/call_guard_main.cpp builds a handle on the host over a fake device and runs the guard
with bodies that return, throw ArgError, OptionError, DeviceOOM, std::bad_alloc, HipError and a plain std::runtime_error.  It
checks the status and the exact text on the handle for each, that a DeviceOOM is not taken for a HipError, that no text of an
earlier failure shows in a later one, and that the mutex is free after every call.  Built with AddressSanitizer and UBSan and
run as a program of its own."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_guard_statuses_texts_and_lock_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "call_guard_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-o", exe,
                           os.path.join(HERE, "call_guard_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    last = r.stdout.strip().split("\n")[-1]
    assert last.startswith("ok: ") and last.endswith(", 0 failed"), last
    assert int(last.split()[1]) >= 90   # every arm was reached: the program counts its checks


def test_api_check_turns_a_status_into_the_exception_each_site_raised():
    """lexicmap_amd.api._check: the class, the message and e.status of the forms the binding's sites use"""
    import pytest

    from lexicmap_amd import api

    fetched = []

    def text():
        fetched.append(1)
        return "the_call: keys is NULL but nkeys is not 0"

    assert api._check(0, text) is None and not fetched          # success fetches no text
    for st, refused, fmt, cls, msg in [
            (7, api.REFUSED_ARG, None, ValueError, "the_call: keys is NULL but nkeys is not 0"),
            (3, api.REFUSED_ARG_OR_OPTION, None, ValueError, "the_call: keys is NULL but nkeys is not 0"),
            (3, api.REFUSED_ARG, None, RuntimeError, "liblexicmap_hip error 3: the_call: keys is NULL but nkeys is not 0"),
            (7, (), None, RuntimeError, "liblexicmap_hip error 7: the_call: keys is NULL but nkeys is not 0"),
            (5, api.REFUSED_ARG_OR_OPTION, None, RuntimeError, "liblexicmap_hip error 5: the_call: keys is NULL but nkeys is not 0"),
            (2, api.REFUSED_ARG, "lm_x failed (%(status)d): %(text)s", RuntimeError, "lm_x failed (2): the_call: keys is NULL but nkeys is not 0"),
            (7, api.REFUSED_ARG, "lm_x failed (%(status)d): %(text)s", ValueError, "the_call: keys is NULL but nkeys is not 0"),
            (4, (), "lm_format_rows failed (%(status)d)", RuntimeError, "lm_format_rows failed (4)"),
            (4, (), "lm_pairs_from_rows: status %(status)d", RuntimeError, "lm_pairs_from_rows: status 4")]:
        with pytest.raises(cls) as ei:
            if fmt is None:
                api._check(st, text, refused=refused)
            else:
                api._check(st, text, fmt, refused)
        assert type(ei.value) is cls and str(ei.value) == msg and ei.value.status == st
    with pytest.raises(RuntimeError) as ei:
        api._check(1, "a plain text")                           # the text need not be a callable
    assert str(ei.value) == "liblexicmap_hip error 1: a plain text" and ei.value.status == 1
