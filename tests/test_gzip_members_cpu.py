"""CPU checks of the host side of zng_rocm_gunzip_members_dev (every member of a device-resident gzip file, BGZF included):
the rules of zlib-ng_amd/csrc/gzip_members_plan.h and the BSIZE walk of framing_parse.h, through a small C++ driver
(tests/c/gzip_members_driver.cpp) built here with g++.

  a candidate           src[p .. p + 3] is 1f 8b 08 F with F & 0xe0 == 0 (oracle: an overlapping regular expression)
  BSIZE                 FEXTRA subfield SI1 66 SI2 67 SLEN 2; the member is BSIZE + 1 bytes long
  next(i)               the candidate at pos + BSIZE + 1 (or the end of the file) when BSIZE was given and one is there, else i + 1
  the plan              the chain from a candidate along next; ISIZE guesses summed into dst_off, every member's capacity exactly
                        its guess; spans below 128 KiB engine 0 (one wavefront), others engine 1 (the large batch); the chain stops
                        in front of a candidate whose header was refused or cut, that has no trailer to guess from, whose guess
                        passes 1032 x span or what is left of dst_cap, or whose span reaches 2 GiB: that one is decoded alone
  verification          status 1, out_len == guess, in_used == span (the member guessed to reach the end of the file: <= span)
  behind a member       fewer than 2 bytes or no 1f 8b: garbage (gz_look asks avail_in > 1); 1f 8b: a member that has to decode

Every expected value of the hand-built tables is worked out from these rules; the tables of real files are checked against a
Python loop of zlib.decompressobj(31) over unused_data."""
import glob
import importlib
import json
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np
import pytest

from gzip_files import BGZF_EOF, SCAN, bgzf_block, bgzf_file, oracle_members, zero_free_stored_member
from wrapped_members import gzip_file, handmade, raw, trailer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZF, TRAILER = 1, 2                              # CandRow::flags
KiB = 1 << 10


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gzip_members_driver")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-O1",
                               "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"),
                               os.path.join(ROOT, "tests", "c", "gzip_members_driver.cpp"), "-o", exe])

        def run(cmd, data=None, words=None):
            if data is not None:
                path = os.path.join(tmp, "input.bin")
                with open(path, "wb") as f:
                    f.write(data)
                out = subprocess.run([exe, cmd, path], capture_output=True, text=True, timeout=120)
            else:
                out = subprocess.run([exe, cmd], input=" ".join(str(w) for w in words), capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (cmd, out.returncode, out.stderr)
            return out.stdout
        yield run


def text(n, seed):
    rng = np.random.default_rng(seed)
    words = [b"alpha", b"beta", b"gamma", b"delta", b"\x1f\x8b\x08\x00", b"epsilon ", b"\n", b"0123456789"]
    return b"".join(words[i] for i in rng.integers(0, len(words), size=n // 5))[:n]


# ---- the scan rule ---------------------------------------------------------------------------------------------------------
def _scan(driver, data):
    return [int(x) for x in driver("scan", data=data).split()]


def test_scan_rule_on_bgzf_concatenated_members_and_random_bytes(driver):
    plain = text(300 * KiB, 1)
    files = {"bgzf": bgzf_file(plain, block=20000),
             "concatenated": gzip_file(plain[:70000], "a.txt") + gzip_file(b"", "") + handmade(plain[70000:]) + gzip_file(plain, "", 0),
             "random": np.random.default_rng(7).integers(0, 256, size=1 << 20, dtype=np.uint8).tobytes(),
             # every flag byte behind 1f 8b 08, overlapping heads, a head cut by the end of the file
             "crafted": b"".join(b"\x1f\x8b\x08" + bytes([f]) for f in range(256)) + b"\x1f\x1f\x8b\x08\x1f\x8b\x08\x00\x1f\x8b\x08",
             "short": b"\x1f\x8b\x08", "empty": b""}
    for name, data in files.items():
        want = [m.start() for m in SCAN.finditer(data)]
        assert _scan(driver, data) == want, name
    assert len(_scan(driver, files["bgzf"])) >= 17                       # 16 blocks and the EOF block, and what the plaintext holds
    crafted = _scan(driver, files["crafted"])
    assert crafted[:32] == [4 * f for f in range(32)] and len(crafted) == 32 + 2, crafted     # flags 00 .. 1f; 1f 8b 08 1f and 1f 8b 08 00


# ---- BSIZE -----------------------------------------------------------------------------------------------------------------
def _bsize(driver, member):
    st, hl, bs = (int(x) for x in driver("bsize", data=member).split())
    return st, hl, bs


def test_bsize_parsing(driver):
    plain = b"pack my box with five dozen liquor jugs\n" * 50
    first = bgzf_block(plain)
    assert _bsize(driver, first) == (0, 18, len(first) - 1)
    # the specification's end-of-file block: 28 bytes, an empty member, BSIZE 27
    assert len(BGZF_EOF) == 28 and zlib.decompressobj(31).decompress(BGZF_EOF) == b"" and bgzf_block(b"")[:18] == BGZF_EOF[:18]
    assert _bsize(driver, BGZF_EOF) == (0, 18, 27)
    second = bgzf_block(plain, extra_front=b"XY" + struct.pack("<H", 3) + b"abc")         # 'BC' in second place
    assert _bsize(driver, second) == (0, 25, len(second) - 1)
    behind = bgzf_block(plain, extra_behind=b"ZZ" + struct.pack("<H", 0))                 # 'BC' first, another behind
    assert _bsize(driver, behind) == (0, 22, len(behind) - 1)

    def member(extra):
        head = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", len(extra)) + extra
        return head + raw(plain) + trailer(2, plain)

    # SLEN != 2: a subfield like any other, skipped; a regular one behind it still counts
    four = b"BC" + struct.pack("<H", 4) + b"\x11\x22\x33\x44"
    assert _bsize(driver, member(four)) == (0, 12 + 8, -1)
    assert _bsize(driver, member(four + b"BC" + struct.pack("<HH", 2, 999))) == (0, 12 + 14, 999)
    # XLEN cuts the subfield short: XLEN 5 ends inside the two bytes of BSIZE, XLEN 3 inside SLEN -- the header is accepted
    # (inflate skips XLEN bytes whatever they hold), and there is no BSIZE
    full = b"BC" + struct.pack("<HH", 2, 777)
    assert _bsize(driver, member(full[:5])) == (0, 17, -1)
    assert _bsize(driver, member(full[:3])) == (0, 15, -1)
    assert _bsize(driver, member(b"XY" + struct.pack("<H", 40) + full)) == (0, 12 + 10, -1)    # a subfield that claims more than XLEN
    # no FEXTRA, an empty one, and a header that is not accepted
    assert _bsize(driver, gzip_file(plain, "name")) == (0, 15, -1)
    assert _bsize(driver, member(b"")) == (0, 12, -1)
    assert _bsize(driver, first[:14])[0] == -5
    for m in (first, second, behind, member(four), member(full[:5])):                      # none of it changes what is decoded
        assert zlib.decompressobj(31).decompress(m) == plain


# ---- the candidate table of real files -------------------------------------------------------------------------------------
def _table(driver, data):
    return [tuple(int(x) for x in line.split()) for line in driver("table", data=data).strip("\n").split("\n") if line]


def _plan(driver, rows, src_len, start=0, dst_off=0, dst_cap=1 << 40, results=()):
    words = [len(rows), src_len, start, dst_off, dst_cap]
    for r in rows:
        words += list(r)
    words.append(len(results))
    for r in results:
        words += list(r)
    lines = driver("plan", words=words).strip("\n").split("\n")
    items, stop, dst_end, unverified = [], None, None, None
    for line in lines:
        w = line.split()
        if w[0] in ("alone", "end"):
            stop = (w[0], int(w[1]), w[2]) if w[0] == "alone" else ("end",)
        elif w[0] == "dst_end":
            dst_end = int(w[1])
        elif w[0] == "unverified":
            unverified = int(w[1])
        else:
            items.append(tuple(int(x) for x in w))
    return items, stop, dst_end, unverified


def test_table_and_plan_of_a_bgzf_file_hop_over_false_candidates(driver):
    plain = text(200 * KiB, 2)                                           # the plaintext is full of 1f 8b 08 00 ...
    blocks = [bgzf_block(plain[at:at + 30000], level=0) for at in range(0, len(plain), 30000)]       # ... and stored blocks keep it
    data = b"".join(blocks) + BGZF_EOF
    members, end = oracle_members(data)
    assert end == len(data) and len(members) == len(blocks) + 1
    rows = _table(driver, data)
    starts = [m[0] for m in members]
    assert len(rows) > 3 * len(members)                                  # most candidates are false
    assert [r[0] for r in rows] == [m.start() for m in SCAN.finditer(data)]
    by_pos = {r[0]: (i, r) for i, r in enumerate(rows)}
    for k, (off, used, p) in enumerate(members):                         # every real member hops to the next real member
        i, r = by_pos[off]
        assert r[3] == 0 and r[1] == 18 and r[5] == BGZF | TRAILER, r
        assert (rows[r[2]][0] if r[2] < len(rows) else len(data)) == off + used
        assert (r[6], r[7]) == (zlib.crc32(p), len(p))
    items, stop, dst_end, _ = _plan(driver, rows, len(data))
    assert stop == ("end",) and dst_end == len(plain)
    assert [(it[2], it[3], it[5], it[6], it[7]) for it in items] == [(off, used, len(p), zlib.crc32(p), 1) for off, used, p in members]
    assert [it[4] for it in items] == [sum(len(m[2]) for m in members[:k]) for k in range(len(members))]
    assert all(it[1] == 0 for it in items) and [it[8] for it in items] == [0] * len(blocks) + [1]


def test_table_and_plan_of_concatenated_members(driver):
    noise = np.random.default_rng(4).integers(0, 256, size=200 * KiB, dtype=np.uint8).tobytes()      # a member of 128 KiB and more
    plains = [b"", b"x", text(100 * KiB, 3).replace(b"\x1f\x8b\x08\x00", b"...."), noise]
    data = gzip_file(plains[0], "") + handmade(plains[1]) + gzip_file(plains[2], "hundred.txt") + gzip_file(plains[3], "", 1)
    members, end = oracle_members(data)
    assert end == len(data) and [m[2] for m in members] == plains
    rows = _table(driver, data)
    assert [r[0] for r in rows] == [m[0] for m in members]               # compressed data rarely holds the four bytes: none here
    items, stop, dst_end, unverified = _plan(driver, rows, len(data), results=[(1, len(p), used) for _, used, p in members])
    assert stop == ("end",) and dst_end == sum(len(p) for p in plains) and unverified == len(members)
    assert [(it[2], it[3], it[5]) for it in items] == [(off, used, len(p)) for off, used, p in members]
    assert [it[1] for it in items] == [0 if used < 128 * KiB else 1 for _, used, _ in members]
    assert [it[1] for it in items].count(1) >= 1 and [it[7] for it in items] == [0] * 4


# ---- hand-built tables ------------------------------------------------------------------------------------------------------
def row(pos, next_, isize=1000, crc=0xC0FFEE, header_len=10, status=0, msg=0, flags=TRAILER):
    return (pos, header_len, next_, status, msg, flags, crc, isize)


def test_chain_hops_over_a_false_candidate_inside_a_bgzf_member(driver):
    # candidates 0 (BGZF, 500 bytes), 1 (inside it), 2 (BGZF, to the end of the file at 900)
    rows = [row(0, 2, isize=4000, flags=BGZF | TRAILER), row(120, 2, isize=77), row(500, 3, isize=0, flags=BGZF | TRAILER)]
    items, stop, dst_end, unverified = _plan(driver, rows, 900, dst_off=64, results=[(1, 4000, 500), (1, 0, 400)])
    assert items == [(0, 0, 0, 500, 64, 4000, 0xC0FFEE, 1, 0), (2, 0, 500, 400, 4064, 0, 0xC0FFEE, 1, 1)]
    assert stop == ("end",) and dst_end == 4064 and unverified == 2


def test_a_false_candidate_with_no_bsize_forces_a_new_plan(driver):
    # the member at 0 really is 700 bytes long; candidate 1 at 300 lies in its data, so the guess is [0, 300) with the "ISIZE"
    # found at 296 -- the engines' answer refutes it: the plan's first member is the first unverified one
    rows = [row(0, 1, isize=123456), row(300, 2, isize=5), row(700, 3, isize=2000)]
    items, stop, _, unverified = _plan(driver, rows, 1000, results=[(-5, 123456, 300), (-3, 0, 4), (1, 2000, 300)])
    assert [it[:4] for it in items] == [(0, 0, 0, 300), (1, 0, 300, 400), (2, 0, 700, 300)] and stop == ("end",)
    assert unverified == 0                                               # ... although the third one's own answer is fine
    # decoded alone, it ended at 700 with 9000 bytes: the new plan starts at the candidate there
    items, stop, dst_end, unverified = _plan(driver, rows, 1000, start=2, dst_off=9000, results=[(1, 2000, 300)])
    assert items == [(2, 0, 700, 300, 9000, 2000, 0xC0FFEE, 0, 1)] and stop == ("end",) and dst_end == 11000 and unverified == 1
    # each way a member can refute its guess
    for res in ((1, 1999, 300), (1, 2001, 300), (1, 2000, 301), (-3, 2000, 300), (-5, 2000, 300), (0, 2000, 300)):
        assert _plan(driver, [row(0, 1, isize=5), row(700, 2, isize=2000)], 1000, results=[(1, 5, 700), res])[3] == 1, res
    # ... but only the member guessed to reach the end of the file may stop short of its span
    assert _plan(driver, [row(0, 1, isize=5), row(700, 2, isize=2000)], 1000, results=[(1, 5, 699), (1, 2000, 300)])[3] == 0
    assert _plan(driver, [row(0, 1, isize=5), row(700, 2, isize=2000)], 1000, results=[(1, 5, 700), (1, 2000, 290)])[3] == 2


def test_trailing_garbage_and_a_single_trailing_1f(driver):
    def after(at, src_len, b0=0, b1=0):
        return driver("after", words=[at, src_len, b0, b1]).strip()

    assert after(1000, 1000) == "done"                                   # the file ends with the member
    assert after(999, 1000, 0x1f, 0x8b) == "done"                        # one byte: gz_look asks avail_in > 1
    assert after(998, 1000, 0x1f, 0x8b) == "member"                      # two bytes 1f 8b: a member, however short
    assert after(900, 1000, 0x1f, 0x8c) == "done" and after(900, 1000, 0x00, 0x8b) == "done" and after(900, 1000, 0x8b, 0x1f) == "done"
    assert after(900, 1000, 0x1f, 0x8b) == "member"
    # the last member of a file with 100 bytes of garbage behind it: its guess reads the garbage's last eight bytes; the engine's
    # answer (the member's real 40 bytes out, 200 in) refutes a guess of 41 and agrees with one of 40
    rows = [row(0, 1, isize=10), row(500, 2, isize=41)]
    assert _plan(driver, rows, 800, results=[(1, 10, 500), (1, 40, 200)])[3] == 1
    rows = [row(0, 1, isize=10), row(500, 2, isize=40)]
    assert _plan(driver, rows, 800, results=[(1, 10, 500), (1, 40, 200)])[3] == 2


def test_a_second_member_whose_header_is_refused_is_decoded_alone(driver):
    # candidate 1's header was refused (-3, message 5 = header crc mismatch) or cut (-5): the chain stops in front of it
    for status, msg in ((-3, 5), (-5, 0)):
        rows = [row(0, 1, isize=10), row(500, 2, status=status, msg=msg, flags=0), row(600, 3, isize=7)]
        items, stop, dst_end, _ = _plan(driver, rows, 800)
        assert [it[0] for it in items] == [0] and stop == ("alone", 1, "must") and dst_end == 10
    # a guess the plan can tell is wrong -- the guessed end lies inside header + trailer (a candidate inside the member), or the
    # length is beyond deflate's 1032 : 1 -- counts as a re-plan ("guess"); a span for the pieces engine does not ("must")
    assert _plan(driver, [row(0, 1, flags=0), row(12, 2)], 800)[1] == ("alone", 0, "guess")
    assert _plan(driver, [row(0, 1, isize=100 * 1032 + 1), row(100, 2)], 800)[1] == ("alone", 0, "guess")
    assert _plan(driver, [row(0, 1, isize=100 * 1032), row(100, 2)], 800)[1] == ("end",)
    assert _plan(driver, [row(0, 1, isize=5), row(1 << 31, 2)], (1 << 31) + 500)[1] == ("alone", 0, "must")
    items, stop, _, _ = _plan(driver, [row(0, 1, isize=5), row((1 << 31) - 1, 2)], (1 << 31) + 500)
    assert stop == ("end",) and [it[1] for it in items] == [1, 0]
    # the cut between the engines: a span of 128 KiB is the large engine's
    items = _plan(driver, [row(0, 1), row(128 * KiB - 1, 2), row(256 * KiB - 1, 3)], 256 * KiB + 99)[0]
    assert [(it[3], it[1]) for it in items] == [(128 * KiB - 1, 0), (128 * KiB, 1), (100, 0)]


def test_dst_cap_one_byte_short(driver):
    rows = [row(0, 1, isize=1000), row(300, 2, isize=2000), row(700, 3, isize=500)]
    items, stop, dst_end, _ = _plan(driver, rows, 1000, dst_cap=3500)
    assert stop == ("end",) and dst_end == 3500 and [(it[4], it[5]) for it in items] == [(0, 1000), (1000, 2000), (3000, 500)]
    items, stop, dst_end, _ = _plan(driver, rows, 1000, dst_cap=3499)    # the third no longer fits: alone, with the 499 bytes left
    assert stop == ("alone", 2, "must") and dst_end == 3000 and [it[0] for it in items] == [0, 1]
    items, stop, dst_end, _ = _plan(driver, rows, 1000, dst_cap=999)
    assert stop == ("alone", 0, "must") and items == [] and dst_end == 0
    items, stop, dst_end, _ = _plan(driver, rows, 1000, start=1, dst_off=1000, dst_cap=2999)
    assert stop == ("alone", 1, "must") and items == [] and dst_end == 1000


# ---- the whole file on the host: table, plan, engines played by CPython ----------------------------------------------------
def _engine(data, item):
    """what an engine says about a planned member: the member decoded from its guessed bytes into its guessed capacity"""
    _, _, off, span, _, guess, _, _, _ = item
    piece = data[off:off + span]
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(piece, guess + 1)
    except zlib.error:
        return (-3, 0, 0)
    if not d.eof or len(out) > guess:
        return (-5, len(out), span)
    return (1, len(out), span - len(d.unused_data))


def _host_gunzip(driver, data):
    """the call's loop with the driver's plan and CPython for the engines -> (members, replans, in_used)"""
    rows = _table(driver, data)
    pos = [r[0] for r in rows]
    at, out, members, replans = 0, 0, [], 0
    while True:
        if at not in pos:
            if members and (len(data) - at < 2 or data[at:at + 2] != b"\x1f\x8b"):
                return members, replans, at
            raise AssertionError("a member in trouble at %d" % at)
        items, stop, _, _ = _plan(driver, rows, len(data), start=pos.index(at), dst_off=out)
        results = [_engine(data, it) for it in items]
        good = _plan(driver, rows, len(data), start=pos.index(at), dst_off=out, results=results)[3] if items else 0
        for it, res in zip(items[:good], results):
            members.append((it[2], res[2], it[4], res[1], it[6], it[7]))
            at, out = it[2] + res[2], it[4] + res[1]
        if good == len(items) and stop == ("end",):
            continue
        replans += good < len(items) or stop[-1] == "guess"
        d = zlib.decompressobj(31)                                       # alone, at its true place
        plain = d.decompress(data[at:])
        assert d.eof
        used = len(data) - at - len(d.unused_data)
        members.append((at, used, out, len(plain), zlib.crc32(plain), 1 if rows[pos.index(at)][5] & BGZF else 0))
        at, out = at + used, out + len(plain)


def test_whole_files_on_the_host(driver):
    inner = gzip_file(text(20 * KiB, 5).replace(b"\x1f\x8b\x08\x00", b"...."), "inner.txt")
    nested = gzip_file(inner, "", 0)                                     # a stored block that holds a complete valid member
    tail = [gzip_file(b"behind the nested one " * 100, ""), handmade(b"the last member\n" * 50)]
    cases = {"nested-then-two": nested + tail[0] + tail[1],
             "nested-as-a-bgzf-block": bgzf_block(inner, level=0) + bgzf_block(b"second block " * 99) + BGZF_EOF,
             "garbage-behind": nested + tail[0] + b"\x00garbage" * 30,
             "one-1f-behind": tail[0] + tail[1] + b"\x1f"}
    expect_replans = {"nested-then-two": 1, "nested-as-a-bgzf-block": 0, "garbage-behind": None, "one-1f-behind": None}
    for name, data in cases.items():
        want, end = oracle_members(data)
        members, replans, used = _host_gunzip(driver, data)
        assert used == end, name
        assert [m[:2] for m in members] == [w[:2] for w in want], name
        assert [(m[3], m[4]) for m in members] == [(len(w[2]), zlib.crc32(w[2])) for w in want], name
        assert [m[2] for m in members] == [sum(len(w[2]) for w in want[:k]) for k in range(len(want))], name
        inside = [p for p in (m.start() for m in SCAN.finditer(data)) if any(o < p < o + n for o, n, _ in want)]
        # a member is decoded alone at most once, and only a candidate inside it -- or, for the last member, garbage behind
        # it, which its guesses are then read from -- can make its guess wrong
        assert replans <= len(inside) + (1 if end < len(data) else 0), (name, replans, inside)
        if expect_replans[name] is not None:
            assert replans == expect_replans[name], (name, replans)
        if name.startswith("nested"):
            assert inside and all(m[0] not in inside for m in members), name


# ---- zng_rocm_wrapper_parse is what it was ----------------------------------------------------------------------------------
def test_wrapper_parse_results_on_the_committed_fixtures_are_unchanged():
    """recorded from the library before framing_parse.h learnt about BSIZE (tests/golden/wrapper_parse_results.json)"""
    importlib.import_module("zlib-ng_amd")
    parse = importlib.import_module("zlib-ng_amd.inflate").wrapper_parse
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "wrapper_parse_results.json")))
    paths = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "*")))
    assert sorted(recorded) == sorted(os.path.basename(p) for p in paths)
    for path in paths:
        data = open(path, "rb").read()
        got = {str(fmt): list(parse(fmt, data)) for fmt in (0, 1, 2)}
        assert got == recorded[os.path.basename(path)], path
    first = bgzf_block(b"a BGZF member through the unchanged entry point")
    assert parse(2, first) == (0, 18, 0, 0, None)


# ---- what discovery may cost on a file made to hurt --------------------------------------------------------------------------
LOOK = 4096                                       # kMembersHeaderLook: the bytes of a candidate the header kernel is shown


def _cost(driver, data):
    candidates, examined = (int(x) for x in driver("cost", data=data).split())
    return candidates, examined


def test_a_zero_free_run_of_fname_candidates_costs_a_bounded_number_of_bytes(driver):
    """1f 8b 08 08 repeated in stored blocks with no zero byte: a candidate every four bytes, each with FNAME set and nothing
    to end the name before the trailer.  Reading every name to its end is (candidates x file / 2) bytes; the header rules are
    shown LOOK bytes of a candidate, so they look at no more than 4 fixed bytes and LOOK bytes of name per candidate -- and
    twice the file is twice the cost, not four times."""
    cost = {}
    for blocks in (8, 16):
        for pattern in (b"\x1f\x8b\x08\x08", b"\x1f\x8b\x08\x1a"):       # FNAME; FNAME, FCOMMENT and FHCRC
            member, _ = zero_free_stored_member(pattern, blocks)
            candidates, examined = _cost(driver, member)
            assert candidates >= blocks * (0x7f7f // 4 - 2)
            assert examined <= candidates * (LOOK + 4), (blocks, pattern, candidates, examined)
            assert examined < candidates * len(member) // 16             # (far from every name read to its end)
            cost[blocks, pattern] = examined
            rows = _table(driver, member)
            assert rows[0][3] == 0 and rows[0][0] == 0                   # the member's own header
            cut = [r for r in rows[1:] if r[0] + LOOK <= len(member) - 8]
            assert len(cut) > candidates - LOOK // 4 - 4 and all(r[3] == -5 for r in cut)
            # the plan: the guess [0, first false candidate) cannot be right, the member is decoded alone
            assert _plan(driver, rows, len(member))[1] == ("alone", 0, "guess")
    for pattern in (b"\x1f\x8b\x08\x08", b"\x1f\x8b\x08\x1a"):
        assert cost[16, pattern] <= 2 * cost[8, pattern] + 2 * LOOK * LOOK


def test_a_header_longer_than_the_look_is_cut_and_its_member_decoded_alone(driver):
    plains = [b"first member\n" * 40, b"the one with a long name\n" * 30, b"third member\n" * 20]
    long_name = handmade(plains[1], name=b"n" * (LOOK + 900))            # FEXTRA, FNAME, FCOMMENT, FHCRC: a legal header of 5 KiB
    fits = handmade(plains[1], name=b"n" * (LOOK - 200))
    for second, status in ((long_name, -5), (fits, 0)):
        data = gzip_file(plains[0], "a") + second + gzip_file(plains[2], "c")
        want, end = oracle_members(data)
        assert end == len(data) and [w[2] for w in want] == plains
        rows = _table(driver, data)
        assert [r[0] for r in rows] == [w[0] for w in want] and [r[3] for r in rows] == [0, status, 0]
        items, stop, _, _ = _plan(driver, rows, len(data))
        assert ([it[0] for it in items], stop) == (([0], ("alone", 1, "must")) if status else ([0, 1, 2], ("end",)))
        members, replans, used = _host_gunzip(driver, data)
        assert used == end and replans == 0 and [m[:2] for m in members] == [w[:2] for w in want]
        assert [(m[3], m[4]) for m in members] == [(len(p), zlib.crc32(p)) for p in plains]
