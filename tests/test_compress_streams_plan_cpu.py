"""CPU checks of the host side of zng_rocm_compress_streams2_dev / zng_rocm_compress_members_dev (many device-resident streams
deflated at any level and strategy and wrapped as raw / zlib / gzip members): the rules of
zlib-ng_amd/csrc/compress_streams_plan.h through a small C++ driver (tests/c/compress_streams_plan_driver.cpp) built here with
g++.

  the zlib header   the two bytes CPython's zlib.compressobj(level, DEFLATED, 15, 8, strategy) begins with, for every level and
                    strategy
  the gzip header   1f 8b 08 00, mtime 0, XFL 2 at level 9, else 4 for strategy >= Z_HUFFMAN_ONLY or level < 2, else 0, OS 3
  the trailers      Adler-32 most significant byte first; CRC-32 and ISIZE least significant first
  level 0           blocks of 65535 bytes, 5 bytes of header each, an empty input one empty block, the sync marker's 5 bytes
                    behind a block that is not final
  the rounds        jobs are taken while their plaintext stays within round_bytes (0 = 4 GiB), a job is never split
  the refusals      every one of them, with its status
  the bounds        zng_rocm_deflate_bound + 0 / 6 / 18
Every expected value is worked out here from these rules."""
import os
import struct
import subprocess
import tempfile
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, BUF_ERROR = -3, -5
LEVELS = (-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9)
STRATEGIES = (0, 1, 2, 3, 4)


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "compress_streams_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-O1",
                               "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"),
                               os.path.join(ROOT, "tests", "c", "compress_streams_plan_driver.cpp"), "-o", exe])

        def run(*args):
            out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (args, out.returncode, out.stderr)
            return out.stdout.splitlines()
        yield run


def want_xfl(level, strategy):
    level = 6 if level == -1 else level
    return 2 if level == 9 else 4 if (strategy >= 2 or level < 2) else 0


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_zlib_header_is_cpythons(driver, strategy):
    for level in LEVELS:
        c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
        want = (c.compress(b"abc") + c.flush())[:2]
        info, head = driver("header", 1, level, strategy)
        assert bytes.fromhex(head) == want, (level, strategy)
        lv = 6 if level == -1 else level
        assert int(info.split()[0]) == lv
        assert int(info.split()[1]) == want[1] >> 6 == (0 if strategy >= 2 or lv < 2 else 1 if lv < 6 else 2 if lv == 6 else 3)
        assert want[0] == 0x78 and (want[0] * 256 + want[1]) % 31 == 0 and not want[1] & 0x20


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_gzip_header_and_xfl(driver, strategy):
    for level in LEVELS:
        info, head = driver("header", 2, level, strategy)
        xfl = want_xfl(level, strategy)
        assert bytes.fromhex(head) == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, xfl, 3]), (level, strategy)
        assert int(info.split()[2]) == xfl
    assert want_xfl(9, 2) == 2 and want_xfl(1, 0) == 4 and want_xfl(2, 0) == 0 and want_xfl(6, 3) == 4 and want_xfl(-1, 1) == 0


def test_raw_has_no_wrapper_and_levels_outside_are_refused(driver):
    assert driver("header", 0, 6, 0) == ["6 2 0", ""] and driver("trailer", 0, 1, 1) == [""]
    assert driver("header", 1, 10, 0) == ["refused"] and driver("header", 1, -2, 0) == ["refused"]


@pytest.mark.parametrize("n", [0, 1, 19, 65535, 76800])
def test_trailer_bytes(driver, n):
    plain = bytes((i * 13 + i // 256) & 0xff for i in range(n))
    assert bytes.fromhex(driver("trailer", 1, zlib.adler32(plain), len(plain))[0]) == struct.pack(">I", zlib.adler32(plain))
    assert bytes.fromhex(driver("trailer", 2, zlib.crc32(plain), len(plain))[0]) == struct.pack("<II", zlib.crc32(plain), len(plain))
    # a whole member put together from the rules decodes
    z = bytes.fromhex(driver("header", 1, 0, 0)[1]) + b"\x01" + struct.pack("<HH", len(plain) & 0xffff, ~len(plain) & 0xffff)
    if len(plain) <= 65535:
        assert zlib.decompress(z + plain + struct.pack(">I", zlib.adler32(plain))) == plain


@pytest.mark.parametrize("n", [0, 1, 65535, 65536, 131070, 131071])
def test_stored_sizes(driver, n):
    blocks = max(1, -(-n // 65535))
    assert blocks == {0: 1, 1: 1, 65535: 1, 65536: 2, 131070: 2, 131071: 3}[n]
    for flags in (0, 1, 2, 3):
        out = driver("stored", n, flags)
        marker = 1 if flags == 3 else 0                                  # the sync marker follows only a block that is not final
        assert [int(x) for x in out[0].split()] == [blocks, n + 5 * blocks + 5 * marker, marker], (n, flags)
        lens = [min(65535, n - b * 65535) for b in range(blocks)]
        assert len(out) == 1 + blocks
        for b, line in enumerate(out[1:]):
            ln, head = line.split()
            final = b == blocks - 1 and not flags & 1
            assert int(ln) == lens[b] and bytes.fromhex(head) == bytes([1 if final else 0]) + struct.pack("<HH", lens[b], lens[b] ^ 0xffff)
    # the stream the rules describe is one CPython inflates
    plain = bytes((i * 11 + i // 251) & 0xff for i in range(n))
    body = b"".join(bytes.fromhex(line.split()[1]) + plain[b * 65535:(b + 1) * 65535] for b, line in enumerate(driver("stored", n, 0)[1:]))
    assert len(body) == n + 5 * blocks and zlib.decompress(body, -15) == plain


def want_rounds(lens, round_bytes):
    room, rounds, first = round_bytes or 4 << 30, [], 0
    while first < len(lens):
        last, total = first, 0
        while last < len(lens) and (last == first or total + lens[last] <= room):
            total += lens[last]
            last += 1
        rounds.append((first, last - first))
        first = last
    return rounds


def test_rounds(driver):
    K = 1 << 10
    lens = [0, 1, 5, 61439, 61440, 61441, 65535, 65536, 131071, 131072, 131073, 200000, 2 * 131072 + 17, 65536, 1000]
    for rb in (0, 1, 256 * K, 131073, 131072, 10 ** 9):
        out = driver("rounds", rb, *lens)
        want = want_rounds(lens, rb)
        assert int(out[0]) == len(want) and [tuple(int(x) for x in line.split()) for line in out[1:]] == want, rb
        assert sum(n for _, n in want) == len(lens) and all(n >= 1 for _, n in want)
    assert want_rounds(lens, 0) == [(0, len(lens))] == want_rounds(lens, 10 ** 9)
    # round_bytes 1: a job of one byte takes the empty jobs around it along, a longer one is alone
    assert want_rounds([0, 1, 0, 0, 7, 0], 1) == [(0, 4), (4, 1), (5, 1)]
    assert [tuple(int(x) for x in line.split()) for line in driver("rounds", 1, 0, 1, 0, 0, 7, 0)[1:]] == [(0, 4), (4, 1), (5, 1)]
    # a job larger than round_bytes is a round of its own
    w = want_rounds(lens, 256 * K)
    assert (12, 1) in w and lens[12] > 256 * K
    assert driver("rounds", 100) == ["0"]                                # no jobs, no rounds
    assert driver("rounds", 0, 0xf0000000, 0xf0000000) == ["2", "0 1", "1 1"]          # the default is 4 GiB


def test_call_refusals(driver):
    def call(fmt=2, level=6, strategy=0, jobs=1, njobs=3, results=1):
        return int(driver("call", fmt, level, strategy, jobs, njobs, results)[0])
    assert call() == 0
    assert all(call(fmt=f) == 0 for f in (0, 1, 2)) and all(call(level=v) == 0 for v in LEVELS)
    assert all(call(strategy=s) == 0 for s in STRATEGIES)
    for bad in (dict(fmt=-1), dict(fmt=3), dict(level=-2), dict(level=10), dict(strategy=-1), dict(strategy=5), dict(jobs=0),
                dict(results=0)):
        assert call(**bad) == EINVAL, bad
    assert call(jobs=0, njobs=0, results=0) == 0                         # njobs == 0 returns 0
    assert call(fmt=3, njobs=0) == EINVAL
    assert driver("file", 1, 100) == ["0"] and driver("file", 0, 0) == ["0"] and driver("file", 1, 0) == ["0"]
    assert driver("file", 0, 1) == [str(EINVAL)]


def bound(n, fmt):
    nseg = max(1, -(-n // (128 << 10)))
    return n + n // 8 + nseg * 1032 + 16 + (0, 6, 18)[fmt]


def test_job_refusals(driver):
    def job(fmt=0, per_job=1, have_in=1, in_len=1000, have_out=1, out_cap=None, dict_len=0, flags=0):
        cap = bound(in_len, fmt) if out_cap is None else out_cap
        return int(driver("job", fmt, per_job, have_in, in_len, have_out, cap, dict_len, flags)[0])
    assert all(job(fmt=f) == 0 for f in (0, 1, 2))
    assert job(dict_len=32768) == 0 and job(dict_len=32769) == EINVAL
    assert all(job(flags=f) == 0 for f in (0, 1, 2, 3)) and job(flags=4) == EINVAL and job(flags=0x80000000) == EINVAL
    for fmt in (1, 2):                                                   # a wrapped format takes neither
        assert job(fmt=fmt, dict_len=1) == EINVAL and job(fmt=fmt, flags=1) == EINVAL and job(fmt=fmt, flags=2) == EINVAL
    assert job(have_in=0) == EINVAL and job(have_in=0, in_len=0) == 0 and job(have_in=0, in_len=0, dict_len=1) == EINVAL
    assert job(have_out=0) == EINVAL and job(have_out=0, per_job=0, out_cap=0) == 0
    for fmt in (0, 1, 2):                                                # out_cap one below the bound
        assert job(fmt=fmt, out_cap=bound(1000, fmt) - 1) == BUF_ERROR and job(fmt=fmt, per_job=0, out_cap=0) == 0
    # the bound must fit 32 bits: the largest in_len that does, and the next
    lo, hi = 0, 0xffffffff
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if bound(mid, 2) <= 0xffffffff else (lo, mid - 1)
    assert job(fmt=2, per_job=0, in_len=lo, out_cap=0) == 0 and job(fmt=2, per_job=0, in_len=lo + 1, out_cap=0) == EINVAL
    assert job(fmt=0, per_job=0, in_len=0xffffffff, out_cap=0) == EINVAL
    # the first refusal in job order decides
    assert driver("jobs", 1, 1, bound(1000, 1), 10, 1000, 5000, 20) == ["%d 2" % BUF_ERROR]
    assert driver("jobs", 1, 1, bound(5000, 1), 10, 1000, 5000, 20) == ["0 -1"]
    assert driver("jobs", 1, 0, 0, 10, 1000, 0xffffffff, 20) == ["%d 2" % EINVAL]


@pytest.mark.parametrize("n", [0, 1, 1000, 131072, 131073, 1 << 20, (1 << 30) + 5])
def test_bounds(driver, n):
    for fmt in (0, 1, 2):
        assert [int(x) for x in driver("bound", n, fmt)[0].split()] == [bound(n, 0), bound(n, fmt)]
        # what level 0 writes fits, with the marker
        assert n + 5 * max(1, -(-n // 65535)) + 5 + (0, 6, 18)[fmt] <= bound(n, fmt)
