"""CPU checks of the host side of the inflate index (zng_rocm_inflate_index_build_dev, _read_dev, _export, _import_dev): the
rules of zlib-ng_amd/csrc/inflate_index_plan.h through a small C++ driver (tests/c/inflate_index_plan_driver.cpp), and the
candidates walk_chain records (inflate_large_plan.h) through a second one (tests/c/inflate_index_chain_driver.cpp), both built
here with g++ -Wall -Wextra -Werror.

  selection    point 0 always; a candidate becomes a point when its out_off is at least the span past the last point and in
               front of plain_len -- with empty blocks, a candidate at plain_len, candidates that arrive per piece (the stop of
               one piece repeated as the first part of the next), and spans smaller than any gap
  the plan     against a model written here: every byte of every clipped range covered exactly once by a direct job or a
               slice, nothing outside a destination, an edge span once per round with out_cap = the furthest need, rounds
               within scratch_bytes unless one range alone is larger, a range never split
  the results  the verdict on a job; the FIRST failing span of a range decides status, msg and out_len
  the blob     a round trip of the rows, and every refused case
  the chain    the candidates are the visited starts with key 0 at the prefix sums of the parts' symbol counts; copies,
               produced, end_bit and final do not depend on the recording
Every expected value is worked out here from these rules."""
import os
import random
import struct
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISMATCH, TOO_LONG = -1, -2
(BLOB_OK, BLOB_SHORT, BLOB_MAGIC, BLOB_VERSION, BLOB_FORMAT, BLOB_SPAN, BLOB_COUNT, BLOB_POINT0, BLOB_IN_BIT, BLOB_OUT_OFF,
 BLOB_WINDOW, BLOB_RESERVED, BLOB_INSIDE, BLOB_SIZE) = range(14)
ROUND_JOBS = 1 << 22


def build(tmp, name):
    exe = os.path.join(tmp, name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-O1",
                           "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"), os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe])
    return exe


def run_numbers(exe, args, numbers):
    flat = []
    for v in numbers:
        flat.extend(v if isinstance(v, (list, tuple)) else [v])
    out = subprocess.run([exe] + args, input=" ".join(str(int(v)) for v in flat), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (args, out.returncode, out.stderr)
    return [[int(x) if x.lstrip("-").isdigit() else x for x in line.split()] for line in out.stdout.splitlines()]


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, "inflate_index_plan_driver")
        yield lambda cmd, *numbers: run_numbers(exe, [cmd], numbers)


@pytest.fixture(scope="module")
def chain_driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(tmp, "inflate_index_chain_driver")
        yield lambda *numbers: run_numbers(exe, [], numbers)


def window_len(out_off):
    return min(32768, out_off)


# ---- limits ---------------------------------------------------------------------------------------------------------------
def test_span_and_scratch_limits(driver):
    assert [driver("span", v)[0][0] for v in (0, 65535, 65536, 1 << 20, 1 << 30, (1 << 30) + 1, 1)] == \
        [1 << 20, 0, 65536, 1 << 20, 1 << 30, 0, 0]
    assert [driver("scratch", v)[0][0] for v in (0, (1 << 20) - 1, 1 << 20, 4 << 30, (4 << 30) + 1)] == \
        [256 << 20, 0, 1 << 20, 4 << 30, 0]


# ---- selection ------------------------------------------------------------------------------------------------------------
def model_select(cands, span, plain_len, header_len):
    pts = [(8 * header_len, 0, 0)]
    for bit, out in cands:
        if out >= pts[-1][1] + span and out < plain_len and bit > pts[-1][0]:
            pts.append((bit, out, window_len(out)))
    return pts


def select(driver, cands, span, plain_len, header_len):
    return [tuple(r) for r in driver("select", span, plain_len, header_len, len(cands), *cands)]


def test_select_point0_alone(driver):
    assert select(driver, [], 65536, 1000, 10) == [(80, 0, 0)]
    assert select(driver, [], 65536, 0, 0) == [(0, 0, 0)]
    # the stream's own first block start is point 0 already
    assert select(driver, [(80, 0)], 65536, 1000, 10) == [(80, 0, 0)]


def test_select_empty_blocks_share_an_out_off(driver):
    # three block starts at the same output offset (two empty blocks): the first that qualifies is taken, the others fall
    # to the span test like any candidate that is too near
    cands = [(16, 0), (5000, 70000), (5010, 70000), (5020, 70000), (9000, 140000)]
    assert select(driver, cands, 65536, 200000, 2) == [(16, 0, 0), (5000, 70000, 32768), (9000, 140000, 32768)]


def test_select_candidate_at_plain_len(driver):
    # the start of an empty final block lies AT plain_len: there is no byte it could serve
    cands = [(0, 0), (4000, 70000), (9000, 140000)]
    assert select(driver, cands, 65536, 140000, 0) == [(0, 0, 0), (4000, 70000, 32768)]
    assert select(driver, cands, 65536, 140001, 0) == [(0, 0, 0), (4000, 70000, 32768), (9000, 140000, 32768)]


def test_select_candidates_per_piece(driver):
    # two pieces: the stop of the first (bit 30000) arrives as the loop's block start AND as the second pass's first part;
    # a host-decoded stretch steps back to a start already seen.  The greedy walk gives what one ordered list gives.
    piece1 = [(0, 0), (10000, 66000), (20000, 132000)]
    between = [(30000, 198000)]
    piece2 = [(30000, 198000), (40000, 264000), (50000, 330000)]
    again = [(20000, 132000), (45000, 300000)]
    cands = piece1 + between + piece2 + again + [(60000, 400000)]
    want = [(0, 0, 0), (10000, 66000, 32768), (20000, 132000, 32768), (30000, 198000, 32768), (40000, 264000, 32768),
            (50000, 330000, 32768), (60000, 400000, 32768)]
    assert select(driver, cands, 65536, 500000, 0) == want
    assert select(driver, cands, 65536, 500000, 0) == model_select(cands, 65536, 500000, 0)
    # a span of two gaps: every second one
    assert select(driver, cands, 131072, 500000, 0) == [want[0], want[2], want[4], want[6]]


def test_select_spans_smaller_than_any_gap(driver):
    # gaps of 100000: with a span of 65536 every candidate is a point, and a short window is the offset itself
    cands = [(1000 * k, 100000 * k) for k in range(1, 8)] + [(500, 20000)]
    pts = select(driver, [(500, 20000)] + cands[:-1], 65536, 10 ** 6, 0)
    assert pts == [(0, 0, 0)] + [(1000 * k, 100000 * k, 32768) for k in range(1, 8)]
    assert select(driver, [(500, 70000)], 65536, 10 ** 6, 0) == [(0, 0, 0), (500, 70000, 32768)]
    assert model_select([(500, 20000)], 16384, 10 ** 6, 0)[1] == (500, 20000, 20000)      # (the window rule itself)


def test_select_random_against_model(driver):
    rng = random.Random(5)
    for _ in range(20):
        plain_len = rng.randrange(1, 1 << 24)
        out, bit, cands = 0, 0, []
        for _ in range(rng.randrange(0, 200)):
            out += rng.choice([0, 0, 1, 30000, 70000, 200000])
            bit += rng.randrange(1, 50000)
            cands.append((bit, out))
            if rng.random() < 0.1:
                cands.append((bit, out))
        span = rng.choice([65536, 100000, 1 << 20])
        header = rng.randrange(0, 40)
        cands = [(b + 8 * header, o) for b, o in cands]
        assert select(driver, cands, span, plain_len, header) == model_select(cands, span, plain_len, header)


# ---- the plan -------------------------------------------------------------------------------------------------------------
def parse_plan(out):
    head, clipped = out[0], out[1]
    jobs = [tuple(r[1:]) for r in out[2:] if r[0] == "J"]        # span slot out_cap at range
    parts = [tuple(r[1:]) for r in out[2:] if r[0] == "P"]       # range job at off len slice
    rounds = [tuple(r[1:]) for r in out[2:] if r[0] == "R"]      # range_begin range_end job_begin job_end part_begin part_end slot_bytes slices
    assert head[2:] == [len(jobs), len(parts), len(rounds)]
    return head[0], head[1], clipped, jobs, parts, rounds


def plan(driver, pts, plain_len, ranges, scratch=1 << 20, round_jobs=ROUND_JOBS):
    return parse_plan(driver("plan", plain_len, scratch, round_jobs, len(pts), len(ranges), *pts, *ranges))


def up16(v):
    return (v + 15) & ~15


def check_plan(pts, plain_len, ranges, scratch, got):
    """the properties the read call relies on, from the plan's own tables and the point table"""
    decoded, direct, clipped, jobs, parts, rounds = got
    ends = [p[1] for p in pts[1:]] + [plain_len]
    assert clipped == [0 if u >= plain_len else min(n, plain_len - u) for u, n in ranges]
    # every byte of every clipped range exactly once, in order, from the right place of the right span
    at = {}
    for rng_i, job, pat, off, length, slice_ in parts:
        assert length > 0
        assert pat == at.get(rng_i, 0), "parts of a range are contiguous and in order"
        at[rng_i] = pat + length
        uoff = ranges[rng_i][0]
        assert job >= 0
        span = jobs[job][0]
        assert pts[span][1] + off == uoff + pat, "the span's byte is the range's byte"
        assert pts[span][1] + off + length <= ends[span]
        if slice_:
            assert jobs[job][1] >= 0 and off + length <= jobs[job][2], "a slice lies inside what its edge job decodes"
        else:
            assert jobs[job][1] == -1 and off == 0 and length == jobs[job][2] == ends[span] - pts[span][1]
            assert jobs[job][3] == pat and jobs[job][4] == rng_i
    for i, c in enumerate(clipped):
        assert at.get(i, 0) == c, "covered exactly"
    assert direct == sum(1 for j in jobs if j[1] == -1) and decoded == len(jobs)
    # rounds: contiguous, ranges never split, an edge span once per round with the furthest need, slots apart, within scratch
    jb = pb = 0
    rb = 0
    for r0, r1, j0, j1, p0, p1, slot_bytes, slices in rounds:
        assert (j0, p0) == (jb, pb) and r0 >= rb and r1 > r0 and j1 > j0
        jb, pb, rb = j1, p1, r1
        assert all(r0 <= p[0] < r1 for p in parts[p0:p1]), "a range's parts stand in one round"
        edges = {}
        for j in range(j0, j1):
            if jobs[j][1] != -1:
                assert jobs[j][0] not in edges, "an edge span appears once per round"
                edges[jobs[j][0]] = j
        need = {}
        for p in parts[p0:p1]:
            if p[5]:
                assert j0 <= p[1] < j1
                need[p[1]] = max(need.get(p[1], 0), p[3] + p[4])
        assert slices == sum(1 for p in parts[p0:p1] if p[5])
        off = 0
        for j in range(j0, j1):
            if jobs[j][1] == -1:
                continue
            assert jobs[j][2] == need[j], "an edge is decoded as far as it is used and no further"
            assert jobs[j][1] == off
            off += up16(jobs[j][2])
        assert slot_bytes == off
        nranges_with_parts = len({p[0] for p in parts[p0:p1]})
        assert slot_bytes <= scratch or nranges_with_parts == 1, "only a range that is larger alone passes scratch_bytes"
    assert (jb, pb) == (len(jobs), len(parts))


def test_plan_small_by_hand(driver):
    pts = [(80, 0, 0), (9000, 70000, 32768), (20000, 140000, 32768)]
    ranges = [(0, 10), (69990, 20), (60000, 100000), (299999, 5), (400000, 1), (69000, 2000)]
    got = plan(driver, pts, 300000, ranges)
    decoded, direct, clipped, jobs, parts, rounds = got
    assert clipped == [10, 20, 100000, 1, 0, 2000]
    # span 0 is cut by ranges 0, 1, 2 and 5: ONE job, decoded to byte 70000 (ranges 1, 2 and 5 reach its end)
    assert jobs[0] == (0, 0, 70000, 0, 0)
    # span 1 lies wholly inside range 2: direct, at 10000 of its destination, 70000 bytes
    assert (1, -1, 70000, 10000, 2) in jobs
    # span 1 is also cut by ranges 1 and 5 (to 70010, to 71000): one edge job with the furthest need
    assert [j for j in jobs if j[0] == 1 and j[1] != -1] == [(1, up16(70000), 1000, 0, 0)]
    # span 2 is cut by range 2 (its first 20000 bytes) and range 3 (one byte at 159999 of it)
    assert [j for j in jobs if j[0] == 2] == [(2, up16(70000) + up16(1000), 160000, 0, 0)]
    assert (decoded, direct, len(rounds)) == (4, 1, 1)
    check_plan(pts, 300000, ranges, 1 << 20, got)


def test_plan_random_against_properties(driver):
    rng = random.Random(11)
    for trial in range(25):
        n = rng.randrange(1, 30)
        out, bit, pts = 0, rng.randrange(0, 200), [None]
        pts[0] = (bit, 0, 0)
        for _ in range(n - 1):
            out += rng.choice([65536, 70001, 150000, 1 << 20])
            bit += rng.randrange(100, 10 ** 6)
            pts.append((bit, out, window_len(out)))
        plain_len = out + rng.choice([1, 15, 65536, 500000])
        ranges = []
        for _ in range(rng.randrange(1, 60)):
            length = rng.choice([0, 1, 15, 16, 17, 4095, 65536, 300000, 3 << 20])
            uoff = rng.randrange(0, plain_len + 100000)
            ranges.append((uoff, length))
        if trial % 3 == 0:                                  # many ranges that cut the same spans
            k = rng.randrange(0, n)
            ranges += [(pts[k][1] + rng.randrange(0, 1000), rng.randrange(1, 5000)) for _ in range(10)]
        scratch = rng.choice([1 << 20, 2 << 20, 256 << 20])
        check_plan(pts, plain_len, ranges, scratch, plan(driver, pts, plain_len, ranges, scratch))


def test_plan_rounds_respect_scratch(driver):
    # ten spans of 1 MiB, ranges that each cut one span in its middle and need 600 KiB of it: one slot fits 1 MiB, two do not
    pts = [(1000 * k, (1 << 20) * k, window_len((1 << 20) * k)) for k in range(10)]
    plain_len = 10 << 20
    ranges = [((1 << 20) * k + 500000, 100000 + 14400) for k in range(10)]
    got = plan(driver, pts, plain_len, ranges, 1 << 20)
    assert len(got[5]) == 10 and all(r[6] == up16(614400) for r in got[5])
    check_plan(pts, plain_len, ranges, 1 << 20, got)
    # the same ranges over ONE span share its job and its round
    same = [(500000, 100000 + 14400)] * 10
    got = plan(driver, pts, plain_len, same, 1 << 20)
    assert len(got[5]) == 1 and got[0] == 1 and got[5][0][7] == 10
    # a range whose own two edges are larger than scratch_bytes is a round of its own, and is not split
    wide = [(100, 10), ((1 << 20) - 10, (2 << 20) + 20), (200, 10)]
    got = plan(driver, pts, plain_len, wide, 1 << 20)
    assert [(r[0], r[1]) for r in got[5]] == [(0, 1), (1, 2), (2, 3)]
    check_plan(pts, plain_len, wide, 1 << 20, got)
    # a round closes behind the range that takes it past round_jobs jobs
    got = plan(driver, pts, plain_len, [(0, plain_len), (0, plain_len)], 1 << 20, round_jobs=10)
    assert len(got[5]) == 2 and got[1] == 20


def test_plan_span_too_long_has_no_job(driver):
    pts = [(0, 0, 0), (800, 1 << 32, 32768)]
    plain_len = (1 << 32) + 1000
    ranges = [(100, 50), ((1 << 32) - 10, 20), ((1 << 32) + 5, 10)]
    decoded, direct, clipped, jobs, parts, rounds = plan(driver, pts, plain_len, ranges)
    assert clipped == [50, 20, 10]
    assert parts[0] == (0, -1, 0, 100, 50, 0) and parts[1] == (1, -1, 0, (1 << 32) - 10, 10, 0)
    assert parts[2][:2] == (1, 0) and parts[2][2] == 10
    assert jobs == [(1, 0, 15, 0, 0)] and len(rounds) == 1


# ---- results --------------------------------------------------------------------------------------------------------------
def test_job_verdict(driver):
    assert driver("verdict", 1000, 77, 1, 0, 1000)[0] == [1, 0]
    assert driver("verdict", 999, 77, 1, 0, 1000)[0] == [-3, MISMATCH]           # the stream ended in front of the span's end
    assert driver("verdict", 10, 77, -5, 12, 1000)[0] == [-5, 0]
    assert driver("verdict", 0, 2, -3, 1, 1000)[0] == [-3, 1]


def test_first_failing_span_decides(driver):
    # parts (job, at); verdicts (status, msg)
    ok, bad_type, starved, too_far = (1, 0), (-3, 1), (-5, 0), (-3, 11)
    parts = [(0, 0), (1, 100), (2, 300), (3, 700)]
    assert driver("result", 1000, 4, 4, *parts, ok, ok, ok, ok)[0] == [1, 1000, 0]
    assert driver("result", 1000, 4, 4, *parts, ok, starved, bad_type, ok)[0] == [-5, 100, 0]
    assert driver("result", 1000, 4, 4, *parts, ok, too_far, bad_type, starved)[0] == [-3, 100, 11]
    assert driver("result", 1000, 4, 4, *parts, bad_type, ok, ok, ok)[0] == [-3, 0, 1]
    assert driver("result", 1000, 4, 4, *parts, ok, ok, ok, starved)[0] == [-5, 700, 0]
    # a part on a span of 2 GiB and more: -5 with the "too long" message, wherever it stands
    assert driver("result", 1000, 2, 1, (-1, 0), (0, 500), ok)[0] == [-5, 0, TOO_LONG]
    assert driver("result", 1000, 2, 1, (0, 0), (-1, 500), ok)[0] == [-5, 500, TOO_LONG]
    assert driver("result", 0, 0, 0)[0] == [1, 0, 0]


# ---- the blob -------------------------------------------------------------------------------------------------------------
HEAD, ROW = 56, 24
PTS = [(80, 0, 0), (9000, 20000, 20000), (20000, 140000, 32768)]


def make_blob(driver, fmt=2, header_len=10, src_end=5000, plain_len=300000, span=65536, pts=PTS, windows=None):
    rows = bytes(driver("write", fmt, header_len, src_end, plain_len, span, len(pts), *pts)[0])
    return rows + bytes(sum(p[2] for p in pts) if windows is None else windows)


def check(driver, blob):
    out = driver("check", len(blob), *blob)
    return out[0][0], out[1:]


def test_blob_round_trip_and_layout(driver):
    blob = make_blob(driver)
    assert len(blob) == HEAD + ROW * 3 + 20000 + 32768
    assert struct.unpack_from("<4sIII5Q", blob) == (b"ZRIX", 1, 2, 0, 10, 5000, 300000, 65536, 3)
    assert [struct.unpack_from("<QQII", blob, HEAD + ROW * k) for k in range(3)] == [p + (0,) for p in PTS]
    why, rest = check(driver, blob)
    assert why == BLOB_OK and rest[0] == [2, 10, 5000, 300000, 65536] and [tuple(r) for r in rest[1:]] == PTS
    assert check(driver, make_blob(driver, fmt=0, header_len=0, pts=[(0, 0, 0)], plain_len=0))[0] == BLOB_OK


def patched(blob, at, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, at, value)
    return bytes(b)


def test_blob_every_refused_case(driver):
    blob = make_blob(driver)
    assert check(driver, blob[:HEAD - 1])[0] == BLOB_SHORT
    assert check(driver, b"")[0] == BLOB_SHORT
    assert check(driver, patched(blob, 0, "<I", 0x5849525b))[0] == BLOB_MAGIC
    assert check(driver, patched(blob, 4, "<I", 2))[0] == BLOB_VERSION
    assert check(driver, patched(blob, 4, "<I", 0))[0] == BLOB_VERSION
    assert check(driver, patched(blob, 8, "<I", 3))[0] == BLOB_FORMAT
    assert check(driver, patched(blob, 12, "<I", 1))[0] == BLOB_RESERVED
    assert check(driver, patched(blob, 40, "<Q", 65535))[0] == BLOB_SPAN
    assert check(driver, patched(blob, 40, "<Q", (1 << 30) + 1))[0] == BLOB_SPAN
    assert check(driver, patched(blob, 48, "<Q", 0))[0] == BLOB_COUNT
    assert check(driver, patched(blob, 48, "<Q", 1 << 40))[0] == BLOB_COUNT
    assert check(driver, patched(blob, 16, "<Q", 11))[0] == BLOB_POINT0                      # header_len and point 0 disagree
    assert check(driver, patched(blob, HEAD + 8, "<Q", 1))[0] == BLOB_POINT0
    assert check(driver, patched(blob, HEAD + 16, "<I", 1))[0] == BLOB_POINT0
    assert check(driver, patched(blob, HEAD + ROW, "<Q", 80))[0] == BLOB_IN_BIT               # equal is not ascending
    assert check(driver, patched(blob, HEAD + 2 * ROW, "<Q", 8999))[0] == BLOB_IN_BIT
    assert check(driver, patched(blob, HEAD + 2 * ROW + 8, "<Q", 20000))[0] == BLOB_OUT_OFF
    assert check(driver, patched(blob, 32, "<Q", 140000))[0] == BLOB_OUT_OFF                  # a point at plain_len
    assert check(driver, patched(blob, HEAD + ROW + 16, "<I", 19999))[0] == BLOB_WINDOW
    assert check(driver, patched(blob, HEAD + 2 * ROW + 16, "<I", 32769))[0] == BLOB_WINDOW
    assert check(driver, patched(blob, HEAD + ROW + 20, "<I", 7))[0] == BLOB_RESERVED
    assert check(driver, patched(blob, 24, "<Q", 2499))[0] == BLOB_INSIDE                     # the last point begins at byte 2500
    assert check(driver, patched(blob, 24, "<Q", 2500))[0] == BLOB_OK
    assert check(driver, blob[:-1])[0] == BLOB_SIZE
    assert check(driver, blob + b"\0")[0] == BLOB_SIZE
    assert check(driver, patched(blob, 48, "<Q", 2))[0] == BLOB_SIZE                          # a row fewer: its window is left over
    # one row changed consistently in itself (out_off and window of the middle point) still fails the size
    b = patched(patched(blob, HEAD + ROW + 8, "<Q", 20001), HEAD + ROW + 16, "<I", 20001)
    assert check(driver, b)[0] == BLOB_SIZE


# ---- what walk_chain records ---------------------------------------------------------------------------------------------
NONE = 0xffffffff


def chain_tables(parts, final_last=True):
    """parts: (start bit, key, symbols, next part or None); result words as inflate_streams_kernel<PART> writes them"""
    res, side = [], []
    for i, (start, key, n, nxt) in enumerate(parts):
        end = parts[nxt][0] if nxt is not None else start + 1000
        ended = 1 if nxt is None and final_last else 0
        res += [n, end & 0xffffffff, end >> 32, ended, 0, 0, NONE if nxt is None else nxt, ended]
        handed = 1 if nxt is not None and parts[nxt][1] != 0 else 0
        side += [NONE, 0, 0, 0, handed, 0, 0, 0]
    return res, side


def run_chain(chain_driver, parts, sub, src_len=1 << 20):
    res, side = chain_tables(parts)
    out = chain_driver(len(parts), 0, src_len, 1 if sub else 0, [p[0] for p in parts], [p[1] for p in parts], res, side)
    assert out[2][0] == "cands:"
    cands = out[2][1:]
    return out[0], out[1], list(zip(cands[0::2], cands[1::2]))


def test_chain_candidates_block_starts_only(chain_driver):
    # parts 0 -> 1 -> 3 -> 4 -> 6; 2 and 5 are noise the chain never reaches; 3 begins inside a fixed-code block (key 1), 4
    # inside the dynamic block whose header is at bit 30000 (key 30002)
    parts = [(80, 0, 1000, 1), (10000, 0, 70000, 3), (15000, 0, 5, None), (20000, 1, 300, 4), (31000, 30002, 40000, 6),
             (35000, 0, 9, None), (50000, 0, 2000, None)]
    plain, recorded, cands = run_chain(chain_driver, parts, sub=True)
    assert plain == recorded, "copies, produced, end_bit and final do not depend on the recording"
    assert plain[:4] == ["ok", 1000 + 70000 + 300 + 40000 + 2000, 51000, 1]
    assert plain[4:] == ["0:0:1000", "1:1000:70000", "3:71000:300", "4:71300:40000", "6:111300:2000"]
    # the visited starts with key 0, at the prefix sums of the parts' symbol counts
    assert cands == [(80, 0), (10000, 1000), (50000, 111300)]


def test_chain_candidates_without_sub(chain_driver):
    # no keys are read without SUBBLOCK: every visited part is a block start
    parts = [(0, 7, 500, 2), (4000, 7, 1, None), (9000, 7, 0, 3), (9100, 7, 66000, None)]
    plain, recorded, cands = run_chain(chain_driver, parts, sub=False)
    assert plain == recorded and plain[:4] == ["ok", 66500, 10100, 1]
    assert cands == [(0, 0), (9000, 500), (9100, 500)]          # (an empty block: two starts share an out_off)


def test_chain_failed_walk_records_only_what_it_delivered(chain_driver):
    parts = [(0, 0, 500, 1), (4000, 0, 100, 2), (9000, 0, 7, None)]
    res, side = chain_tables(parts)
    res[8 * 2 + 4] = 1                                          # the last part reports "invalid block type"
    out = chain_driver(3, 0, 1 << 20, 0, [p[0] for p in parts], [0, 0, 0], res, side)
    assert out[0] == out[1] and out[0][0] == "fail" and out[0][1] == 600
    assert out[2][1:] == [0, 0, 4000, 500]
