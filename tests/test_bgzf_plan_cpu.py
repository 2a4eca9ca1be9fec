"""CPU checks of the host side of zng_rocm_bgzf_compress_dev (device-resident plaintext written as a BGZF file): the rules of
zlib-ng_amd/csrc/bgzf_plan.h through a small C++ driver (tests/c/bgzf_plan_driver.cpp) built here with g++.

  the cut        a piece every block_bytes bytes (0 = 65280, at most 65280), rounds of round_bytes rounded down to whole
                 pieces and at least one piece
  the bound      src_len + 31 per member + 28
  a member       26 bytes around the payload; the payload is the engine's unless clen > n + 5 or clen > 65510, then the stored
                 form of n + 5 bytes
  the bytes      header, trailer and end-of-file block as gzip_files.bgzf_block / BGZF_EOF build them
Every expected value is worked out here from these rules."""
import os
import struct
import subprocess
import tempfile
import zlib

import pytest

from gzip_files import BGZF_BLOCK, BGZF_EOF, bgzf_block
from wrapped_members import raw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (0, 1, 65279, 65280, 65281, 3 * 65280 + 17)
BLOCKS = (0, 1, 64, 65280)


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bgzf_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-O1",
                               "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"),
                               os.path.join(ROOT, "tests", "c", "bgzf_plan_driver.cpp"), "-o", exe])

        def run(*args):
            out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (args, out.returncode, out.stderr)
            return out.stdout.splitlines()
        yield run


def _want_cut(src_len, block, round_bytes):
    piece = block or BGZF_BLOCK
    lens = [min(piece, src_len - at) for at in range(0, src_len, piece)]
    per = max((round_bytes or (1 << 30) + 65280) // piece, 1)         # the default: 1 GiB and one piece
    rounds = [(first, len(lens[first:first + per]), first * piece, sum(lens[first:first + per])) for first in range(0, len(lens), per)]
    return piece, lens, per, rounds, src_len + 31 * len(lens) + 28


@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("src_len", SIZES)
def test_pieces_rounds_and_bound(driver, src_len, block):
    piece = block or BGZF_BLOCK
    for round_bytes in (0, piece, 2 * piece, 2 * piece + piece // 2 + 1, 1):
        out = driver("cut", src_len, block, round_bytes)
        piece_w, lens, per, rounds, bound = _want_cut(src_len, block, round_bytes)
        assert [int(x) for x in out[0].split()] == [piece_w, len(lens), per, len(rounds), bound], (src_len, block, round_bytes)
        assert [tuple(int(x) for x in line.split()) for line in out[1:1 + len(rounds)]] == rounds
        assert [int(x) for x in out[1 + len(rounds)].split()] == lens
        assert sum(lens) == src_len and all(0 < n <= piece for n in lens)
        if round_bytes in (piece, 2 * piece):                            # rounds of one and of two pieces
            assert per == round_bytes // piece and len(rounds) == -(-len(lens) // per)
        if round_bytes == 1:                                             # less than a piece: still one piece per round
            assert per == 1 and len(rounds) == len(lens)


def test_block_bytes_above_65280_is_refused(driver):
    for src_len in SIZES:
        assert driver("cut", src_len, 65281, 0) == ["refused 0"]
        assert driver("cut", src_len, 0xffffffff, 0) == ["refused 0"]


def test_stored_rule(driver):
    def member(n, clen):
        return tuple(int(x) for x in driver("member", n, clen)[0].split())
    for n in (1, 64, 1000, 65279, 65280):
        assert member(n, n + 5) == (n + 5, 0, n + 31)                    # not larger than the stored form: kept
        assert member(n, n + 6) == (n + 5, 1, n + 31)
        assert member(n, 1) == (1, 0, 27)
    for n in (65279, 65280):                                             # n + 5 < 65510, so the first rule decides here
        assert member(n, 65510) == (n + 5, 1, n + 31)
    # the second rule alone can only decide for a piece above 65280 bytes, which the cut never makes: 65505 is the one length
    # at which both forms weigh 65510
    assert member(65505, 65510) == (65510, 0, 65536)
    assert member(65505, 65511) == (65510, 1, 65536)
    for n in (1, 64, 65280):                                             # level 0: no engine was asked
        assert member(n, 0xffffffff) == (n + 5, 1, n + 31)
    assert max(member(n, c)[2] for n in (1, 65280) for c in (0, n, n + 5, n + 6, 65510, 65511, 1 << 20)) <= 65536


@pytest.mark.parametrize("n, level", [(1, 6), (1000, 1), (65280, 6), (65280, 0), (300, 9)])
def test_header_and_trailer_bytes(driver, n, level):
    plain = bytes((i * 7 + i // 256) & 0xff for i in range(n))
    payload = raw(plain, level)
    want = bgzf_block(plain, level)
    head, tail, stored = (bytes.fromhex(line) for line in driver("frame", len(payload), zlib.crc32(plain), n))
    assert head + payload + tail == want
    assert struct.unpack_from("<H", head, 16)[0] == len(want) - 1
    assert stored == b"\x01" + struct.pack("<HH", n, n ^ 0xffff)
    assert zlib.decompressobj(31).decompress(head[:16] + struct.pack("<H", n + 30) + stored + plain + tail) == plain


def test_end_of_file_block(driver):
    table, by_byte = (bytes.fromhex(line) for line in driver("eof"))
    assert table == BGZF_EOF and by_byte == BGZF_EOF and len(BGZF_EOF) == 28


def test_argument_checks(driver):
    def args(level=6, src=1, src_len=10, block=0, dst=1, cap=100, out=1, members=1, mcap=4, n=1, flags=0):
        return driver("args", level, src, src_len, block, dst, cap, out, members, mcap, n, flags)[0]
    assert args() == "ok 6" and args(level=-1) == "ok 6" and args(level=0) == "ok 0" and args(level=9) == "ok 9"
    assert args(level=1, flags=2) == "ok 1" and args(level=1, flags=3) == "ok 1" and args(flags=1) == "ok 6"
    assert args(src=0, src_len=0) == "ok 6" and args(dst=0, cap=0) == "ok 6" and args(members=0, mcap=0) == "ok 6"
    assert args(block=65280) == "ok 6" and args(block=1) == "ok 6"
    for bad in (dict(level=-2), dict(level=10), dict(flags=4), dict(flags=0x80000000), dict(level=6, flags=2), dict(level=-1, flags=2),
                dict(level=0, flags=2), dict(block=65281), dict(src=0), dict(dst=0), dict(out=0), dict(n=0), dict(members=0)):
        assert args(**bad) == "refused", bad
