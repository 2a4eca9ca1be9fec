"""CPU checks of the host side of zng_rocm_inflate_sizes_dev / zng_rocm_uncompress_packed_dev (many device-resident streams
sized by a parse that stores nothing, and decoded back to back at offsets the device works out): the rules of
zlib-ng_amd/csrc/inflate_sizes_plan.h through a small C++ driver (tests/c/inflate_sizes_plan_driver.cpp) built here with g++.

  the refusals     every one of them, with its status, for both calls
  the count        saturates at 0x7fffffff, the largest room the one-wavefront engine takes
  the sizing row   a refused header, another dictionary's DICTID, the trailer's bytes present and counted, no check compared
  the places       job i starts at the end of the bytes in front of it, rounded up to align (0, 1: back to back); a job whose
                   sizing row is not status 1 takes no room; 64-bit offsets; the last entry is the end of the last job's bytes
  the fit          a job is decoded when it ends at or before dst_cap
  the final rows   case by case
Every expected value is worked out here from these rules."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -3
MAX = 0x7fffffff
# message ids (zng_rocm_inflate_message): 0 none, 1 "invalid block type", 12 "input ended ...", 13 "output buffer too small",
# 14 "incorrect header check", 18 "need dictionary", 19 "incorrect data check"
NONE, BLOCK_TYPE, STARVED, FULL, HEADER_CHECK, NEED_DICT, DATA_CHECK = 0, 1, 12, 13, 14, 18, 19
MISMATCH = 0x80000000                                     # the header verdict "another dictionary"


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "inflate_sizes_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-O1",
                               "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"),
                               os.path.join(ROOT, "tests", "c", "inflate_sizes_plan_driver.cpp"), "-o", exe])

        def run(*args):
            out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (args, out.returncode, out.stderr)
            return out.stdout.splitlines()
        yield run


def test_message_ids_are_the_librarys():
    import importlib
    zr = importlib.import_module("zlib-ng_amd")
    text = lambda i: (zr.lib().zng_rocm_inflate_message(i) or b"").decode()
    assert [text(i) for i in (NONE, BLOCK_TYPE, STARVED, FULL, HEADER_CHECK, NEED_DICT, DATA_CHECK)] == [
        "", "invalid block type", "input ended before the final block", "output buffer too small", "incorrect header check",
        "need dictionary", "incorrect data check"]


def test_call_refusals(driver):
    for fmt in (-1, 3, 100):
        assert driver("call", fmt, 0, 1, 1, 1) == [str(EINVAL)]
    for fmt in (0, 1, 2):
        assert driver("call", fmt, 0, 1, 1, 1) == ["0"]
    assert driver("call", 2, 1, 1, 1, 1) == [str(EINVAL)]                      # gzip has no dictionary
    assert driver("call", 0, 1, 1, 1, 1) == ["0"] and driver("call", 1, 1, 1, 1, 1) == ["0"]
    assert driver("call", 1, 0, 1, 1, 0) == [str(EINVAL)]                      # a null d_results with njobs > 0
    assert driver("call", 1, 0, 0, 1, 1) == [str(EINVAL)]                      # a null job table with njobs > 0
    assert driver("call", 1, 0, 0, 0, 0) == ["0"]                              # njobs == 0 asks for nothing
    assert driver("call", 1, 0, 1, 1 << 31, 1) == [str(EINVAL)]


def test_packed_call_refusals(driver):
    ok = dict(fmt=1, has_dict=0, jobs=1, njobs=3, dst=1, cap=100, align=1, offsets=1, results=1)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return driver("packed", a["fmt"], a["has_dict"], a["jobs"], a["njobs"], a["dst"], a["cap"], a["align"], a["offsets"], a["results"])

    assert call() == ["0"]
    for align in (0, 1, 2, 4, 64, 2048, 4096):
        assert call(align=align) == ["0"]
    for align in (3, 5, 6, 100, 4095, 8192, 1 << 31):
        assert call(align=align) == [str(EINVAL)], align
    assert call(dst=0) == [str(EINVAL)]                                        # a null d_dst with dst_cap > 0
    assert call(dst=0, cap=0) == ["0"]
    assert call(offsets=0) == [str(EINVAL)] and call(results=0) == [str(EINVAL)]
    assert call(offsets=0, njobs=0) == [str(EINVAL)] and call(results=0, njobs=0) == [str(EINVAL)]
    assert call(njobs=0, jobs=0) == ["0"]
    assert call(fmt=3) == [str(EINVAL)] and call(fmt=2, has_dict=1) == [str(EINVAL)] and call(jobs=0) == [str(EINVAL)]


def test_job_refusals(driver):
    def job(fmt=0, has_dict=0, packed=0, have_in=1, in_len=10, dict_len=0, flags=0):
        return driver("job", fmt, has_dict, packed, have_in, in_len, dict_len, flags)

    for fmt in (0, 1, 2):
        for packed in (0, 1):
            assert job(fmt=fmt, packed=packed) == ["0"]
            assert job(fmt=fmt, packed=packed, have_in=0, in_len=0) == ["0"]   # an empty member: its row says so
            assert job(fmt=fmt, packed=packed, have_in=0) == [str(EINVAL)]     # a null buffer with a length
            assert job(fmt=fmt, packed=packed, in_len=MAX) == ["0"]
            assert job(fmt=fmt, packed=packed, in_len=MAX + 1) == [str(EINVAL)]
            assert job(fmt=fmt, packed=packed, flags=1) == [str(EINVAL)] and job(fmt=fmt, packed=packed, flags=1 << 31) == [str(EINVAL)]
    # a history length of the job's own: a raw stream of the sizing call without a dictionary object, at most 32768
    assert job(dict_len=1) == ["0"] and job(dict_len=32768) == ["0"]
    assert job(dict_len=32769) == [str(EINVAL)]
    assert job(dict_len=1, has_dict=1) == [str(EINVAL)]
    assert job(dict_len=1, fmt=1) == [str(EINVAL)] and job(dict_len=1, fmt=2) == [str(EINVAL)]
    assert job(dict_len=1, packed=1) == [str(EINVAL)]                          # a packed buffer has no place for it
    # the first refusal in job order
    assert driver("jobs", 1, 0, 0, 5, 5) == ["0 -1"]
    assert driver("jobs", 1, 0, 0, 3, 5) == ["%d 3" % EINVAL] and driver("jobs", 1, 0, 1, 0, 5) == ["%d 0" % EINVAL]


def test_count_saturates(driver):
    assert driver("add", 0, 1) == ["0 1"] and driver("add", 1000, 258) == ["0 1258"]
    assert driver("add", MAX - 258, 258) == ["0 %d" % MAX]                    # a plaintext of exactly 0x7fffffff bytes still fits
    assert driver("add", MAX - 257, 258) == ["1 %d" % MAX]
    assert driver("add", MAX, 1) == ["1 %d" % MAX] and driver("add", MAX, 0) == ["0 %d" % MAX]
    assert driver("add", MAX - 1, 65535) == ["1 %d" % MAX]


def test_sizing_row_of_a_member(driver):
    def sizing(fmt, hdr, hmsg, in_len, raw):
        return [int(v) for v in driver("sizing", fmt, hdr, hmsg, in_len, *raw)[0].split()]

    # raw: the payload's row is the member's
    assert sizing(0, 0, NONE, 500, (1000, 400, 1, NONE)) == [1000, 400, 1, NONE]
    assert sizing(0, 0, NONE, 500, (7, 30, -3, BLOCK_TYPE)) == [7, 30, -3, BLOCK_TYPE]
    # zlib, 2 header bytes, 4 trailer bytes; gzip, 10 and 8: present -> counted
    assert sizing(1, 2, NONE, 406, (1000, 400, 1, NONE)) == [1000, 406, 1, NONE]
    assert sizing(1, 2, NONE, 500, (1000, 400, 1, NONE)) == [1000, 406, 1, NONE]      # bytes behind the member are not consumed
    assert sizing(2, 10, NONE, 418, (1000, 400, 1, NONE)) == [1000, 418, 1, NONE]
    assert sizing(1, 6, NONE, 410, (1000, 400, 1, NONE)) == [1000, 410, 1, NONE]      # FDICT: 6 header bytes
    # the input ends inside the trailer: -5, as in the decode
    for short in range(1, 5):
        assert sizing(1, 2, NONE, 406 - short, (1000, 400, 1, NONE)) == [1000, 406 - short, -5, STARVED]
    for short in range(1, 9):
        assert sizing(2, 10, NONE, 418 - short, (1000, 400, 1, NONE)) == [1000, 418 - short, -5, STARVED]
    # a fault in the payload: the header's bytes in front of the payload's count
    assert sizing(2, 10, NONE, 418, (7, 30, -3, BLOCK_TYPE)) == [7, 40, -3, BLOCK_TYPE]
    assert sizing(1, 2, NONE, 50, (7, 48, -5, STARVED)) == [7, 50, -5, STARVED]
    # refused headers: nothing consumed; a cut header is -5; another dictionary: -3 without a text, the DICTID consumed
    assert sizing(1, 0, HEADER_CHECK, 418, (0, 0, 0, 0)) == [0, 0, -3, HEADER_CHECK]
    assert sizing(1, 0, NEED_DICT, 418, (0, 0, 0, 0)) == [0, 0, -3, NEED_DICT]
    assert sizing(2, 0, STARVED, 5, (0, 0, 0, 0)) == [0, 0, -5, STARVED]
    assert sizing(1, 6, MISMATCH, 418, (0, 0, 0, 0)) == [0, 6, -3, NONE]


def want_places(align, cap, jobs):
    """the rule, step by step: (offset, room, decoded) per job and the end of the last job's bytes"""
    a = max(align, 1)
    rows, run = [], 0
    for status, size in jobs:
        off = (run + a - 1) // a * a
        room = size if status == 1 else 0
        rows.append((off, room, 1 if status == 1 and off + room <= cap else 0))
        run = off + room
    return rows, run


def places(driver, align, cap, jobs):
    out = driver("places", align, cap, *[v for j in jobs for v in j])
    return [tuple(int(v) for v in line.split()) for line in out[:-1]], int(out[-1])


@pytest.mark.parametrize("align", [0, 1, 2, 64, 4096])
def test_places(driver, align):
    jobs = [(1, 5), (1, 0), (1, 64), (-3, 1000), (1, 1), (-5, 77), (1, 4096), (1, 4097), (1, 0), (1, 63), (-3, 0), (1, 70001)]
    got = places(driver, align, 1 << 40, jobs)
    assert got == want_places(align, 1 << 40, jobs)
    offs = [r[0] for r in got[0]]
    assert all(o % max(align, 1) == 0 for o in offs) and offs == sorted(offs)
    if align <= 1:                                                              # back to back: the sum of the rooms in front
        assert offs == [sum(s for st, s in jobs[:i] if st == 1) for i in range(len(jobs))]
    assert [r[1] for r, j in zip(got[0], jobs) if j[0] != 1] == [0, 0, 0]      # jobs without status 1 take no room
    assert got[1] == offs[-1] + 70001
    # one job, and none
    assert places(driver, align, 100, [(1, 7)]) == ([(0, 7, 1)], 7)
    assert places(driver, align, 100, [(-3, 7)]) == ([(0, 0, 0)], 0)
    assert places(driver, align, 100, []) == ([], 0)
    # offsets above 2^32: five plaintexts of the largest size
    big = [(1, MAX)] * 5 + [(1, 3)]
    got = places(driver, align, 1 << 40, big)
    assert got == want_places(align, 1 << 40, big) and got[0][-1][0] > 1 << 32 and got[1] > 1 << 33


@pytest.mark.parametrize("align", [1, 64])
def test_fit_against_dst_cap(driver, align):
    jobs = [(1, 100), (1, 0), (-3, 50), (1, 200), (1, 0), (1, 30), (1, 1)]
    full, need = want_places(align, 1 << 40, jobs)
    k = 3
    end_k = full[k][0] + full[k][1]
    for cap in (end_k, end_k - 1, end_k + 1, 0, need, need - 1):
        got, got_need = places(driver, align, cap, jobs)
        assert (got, got_need) == want_places(align, cap, jobs)
        assert got_need == need and [g[:2] for g in got] == [f[:2] for f in full]    # the layout does not depend on dst_cap
        fits = [g[2] for g in got]
        if cap == end_k - 1:
            assert fits[k] == 0 and fits[:k] == [1, 1, 0] and not any(fits[k:])       # ... and no job behind it either
        if cap in (end_k, end_k + 1):
            # job k ends at dst_cap or one byte in front of it; the empty plaintext behind it fits only where it starts
            # at or before dst_cap
            assert fits[:k + 1] == [1, 1, 0, 1] and fits[k + 1] == (1 if full[k + 1][0] <= cap else 0) and not any(fits[k + 2:])
        if cap == 0:
            assert not any(fits)                                                      # (the empty plaintext starts behind dst_cap)
        if cap == need:
            assert fits == [1, 1, 0, 1, 1, 1, 1]
        if cap == need - 1:
            assert fits == [1, 1, 0, 1, 1, 1, 0]


def test_final_rows(driver):
    def final(sizing, fits, decoded):
        return [int(v) for v in driver("final", *sizing, fits, *decoded)[0].split()]

    # decoded: its verified row, whatever that says
    assert final((1000, 406, 1, NONE), 1, (1000, 406, 1, NONE)) == [1000, 406, 1, NONE]
    assert final((1000, 406, 1, NONE), 1, (1000, 406, -3, DATA_CHECK)) == [1000, 406, -3, DATA_CHECK]
    # did not fit dst_cap: nothing of the decode's row
    assert final((1000, 406, 1, NONE), 0, (0, 0, -5, STARVED)) == [0, 0, -5, FULL]
    # sizing row not status 1: {0, its in_used, its status, its message}, whether or not anything would fit
    for fits in (0, 1):
        assert final((7, 40, -3, BLOCK_TYPE), fits, (0, 0, -5, STARVED)) == [0, 40, -3, BLOCK_TYPE]
        assert final((900, 300, -5, STARVED), fits, (0, 0, -5, STARVED)) == [0, 300, -5, STARVED]
        assert final((0, 0, -3, HEADER_CHECK), fits, (0, 0, -3, HEADER_CHECK)) == [0, 0, -3, HEADER_CHECK]
        assert final((0, 6, -3, NONE), fits, (0, 6, -3, NONE)) == [0, 6, -3, NONE]
        assert final((MAX, 123, -5, FULL), fits, (0, 0, -5, STARVED)) == [0, 123, -5, FULL]


def test_self_command(driver):
    assert driver("self")[0].startswith("self ok")
