"""CPU checks of the host rules of the rows deflate engine (zng_rocm_deflate_*_dev and everything that compresses through
deflate_blocks.h): zlib-ng_amd/csrc/deflate_rows_plan.h through a small C++ driver (tests/c/deflate_rows_plan_driver.cpp) built
here with g++.

  segment_bytes   512 / 256 / 128 KiB: halved while the stream has fewer than two segments per CU, never below 128 KiB
  the bound       n + n / 8 + 1032 per 128 KiB segment + 16, the same through compress_streams_plan.h
  the table       streams into segments of seg_bytes, segments into blocks at first + k * 61440 (first = the 1024-byte batch that
                  holds the segment's first position; positions count from the first history byte), and every offset, index and
                  mark the kernels read
  the checks      return codes of the block, async and streams calls, their precedence, a call without jobs
  the round cut   with and without the history counted; a job is never split
  the sweep       no block of a stream that has plaintext is without positions, for every dict_len mod 1024
Every expected value is worked out here, by a model of the cut written from these rules; none comes from the driver."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, BUF = 0, -3, -5
KIB = 1024
BATCH, SUB, SEG_MAX, SEG_MIN, PRIME, HIST = 1024, 61440, 512 * KIB, 128 * KIB, 32768, 320
MAX_SUB = (SEG_MAX + BATCH + SUB - 1) // SUB + 1
SEG_JOB, BLK_JOB = 72, 88          # bytes: 3 pointers + 3 x u64 + 6 x u32 (five fields read, the rest zero); 3 pointers + 3 x u64 + 10 x u32
NOT_FINAL, SYNC = 1, 2
LAST = 0x80000000
IN_LENS = (0, 1, 1023, 1024, 1025, 61439, 61440, 61441, 131071, 131072, 131073, 2 * 131072 + 5)
DICT_LENS = (0, 1, 1000, 1024, 32768)


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "deflate_rows_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-O1",
                               "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"),
                               os.path.join(ROOT, "tests", "c", "deflate_rows_plan_driver.cpp"), "-o", exe])

        def run(*args):
            out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (args[:8], out.returncode, out.stderr)
            return out.stdout.splitlines()
        yield run


# ---- the model ------------------------------------------------------------------------------------------------------------------
def bound(n):
    return n + n // 8 + (-(-n // SEG_MIN) if n else 1) * 1032 + 16


def bm_words(n):
    return (n + 2 * BATCH) // 64 + 2


def d16_entries(n):
    return ((n + 2 * BATCH) // 4 + 8) & ~3


def slot_bytes(n):
    return ((n * 9 + 7) // 8 + 1024 + 3) & ~3


def seg_bytes_for(in_len, cus):
    seg = SEG_MAX
    while seg > SEG_MIN and in_len // seg < 2 * cus:
        seg //= 2
    return seg


class Job:
    def __init__(self, in_ptr, out_ptr, in_len, out_cap, dict_len, flags):
        self.args = (in_ptr, out_ptr, in_len, out_cap, dict_len, flags)
        self.in_ptr, self.out_ptr, self.in_len, self.out_cap, self.dict_len, self.flags = self.args


def model(jobs, seg_bytes, shared, rule, cap_one):
    """(segments, blocks) as lists of dicts: the table of the rules in this file's docstring"""
    segs, blks = [], []
    bm = d16 = slot = 0
    for s, j in enumerate(jobs):
        dict_len = shared or j.dict_len
        base = j.in_ptr - dict_len                      # position 0: the first history byte
        first_blk = len(blks)
        cuts = list(range(0, j.in_len, seg_bytes)) or [0]
        for c in cuts:
            a, b = dict_len + c, dict_len + min(c + seg_bytes, j.in_len)
            k = len(segs)
            segs.append(dict(**{"in": base}, bm_off=bm, d16_off=d16, seg_start=a, seg_end=b, unread=0))
            first = a - a % BATCH
            borders = [a] + [p for p in range(first + SUB, b, SUB)] + [b]
            for sub in range(len(borders) - 1):
                blo, bhi = borders[sub], borders[sub + 1]
                cap = 0xffffffffffffffff if rule == 2 else (cap_one if rule == 1 and s == 0 else j.out_cap)
                blks.append(dict(**{"in": base}, out=slot, dst=j.out_ptr, dst_cap=cap, bm_off=bm, d16_off=d16, seg_start=a, seg_end=b,
                                 blo=blo, bhi=bhi, hist_idx=k * MAX_SUB + sub, hist_prev=int(sub > 0), out_cap=slot_bytes(bhi - blo + 258),
                                 is_last=0, first_seg=first_blk, stream=s))
                slot += slot_bytes(bhi - blo + 258)
            bm += bm_words(b - a)
            d16 += d16_entries(b - a)
        blks[-1]["stream"] |= LAST
        blks[-1]["is_last"] = int(not j.flags & NOT_FINAL)
    return segs, blks, (slot, bm, d16)


SEG_FIELDS = ("in", "bm_off", "d16_off", "seg_start", "seg_end", "unread")
BLK_FIELDS = ("in", "out", "dst", "dst_cap", "bm_off", "d16_off", "seg_start", "seg_end", "blo", "bhi", "hist_idx", "hist_prev", "out_cap",
              "is_last", "first_seg", "stream")


def planned(driver, jobs, seg_bytes, shared, rule, cap_one):
    lines = driver("plan", seg_bytes, shared, rule, cap_one, *[v for j in jobs for v in j.args])
    counts = [int(v) for v in lines[0].split()[1:]]
    totals = [int(v) for v in lines[1].split()[1:]]
    segs = [dict(zip(SEG_FIELDS, (int(v) for v in ln.split()[1:]))) for ln in lines if ln.startswith("seg ")]
    blks = [dict(zip(BLK_FIELDS, (int(v) for v in ln.split()[1:]))) for ln in lines if ln.startswith("blk ")]
    assert lines[0].startswith("counts ") and lines[1].startswith("totals ") and len(lines) == 2 + len(segs) + len(blks)
    return counts, totals, segs, blks


def job_list(in_lens, dict_lens, shared):
    """every in_len with every dict_len (none of its own behind a shared window); buffers back to back, room = the bound"""
    jobs, at = [], 1 << 20
    for n in in_lens:
        for d in ((0,) if shared else dict_lens):
            jobs.append(Job(at + d, (1 << 40) + at, n, bound(n), d, NOT_FINAL if (n + d) % 3 == 0 else 0))
            at += d + n + 64
    return jobs


# ---- constants, segment_bytes, the bound ------------------------------------------------------------------------------------------
def test_constants(driver):
    assert [int(v) for v in driver("consts")[0].split()] == [SEG_MAX, SEG_MIN, PRIME, HIST, 60, SUB, MAX_SUB, BATCH, SEG_JOB, BLK_JOB]
    assert MAX_SUB == 10
    for n in (0, 1, 1023, 61440, 131072, 524288):
        assert [int(v) for v in driver("sizes", n)[0].split()] == [bm_words(n), d16_entries(n), slot_bytes(n)]
        # the first batch may begin up to one batch in front: a bit per position, a u16 per four, the emitter's look-ahead
        assert bm_words(n) * 64 >= n + BATCH + 64 and d16_entries(n) * 4 >= n + BATCH and slot_bytes(n) % 4 == 0


@pytest.mark.parametrize("cus", (256, 8, 1))
def test_segment_bytes(driver, cus):
    def got(n):
        return int(driver("segbytes", n, cus)[0])
    # 512 KiB once there are two segments of it per CU, 256 KiB likewise, else 128 KiB
    t512, t256 = 2 * cus * SEG_MAX, 2 * cus * (SEG_MAX // 2)
    assert got(t512) == SEG_MAX and got(t512 - 1) == SEG_MAX // 2
    assert got(t256) == SEG_MAX // 2 and got(t256 - 1) == SEG_MIN
    assert got(0) == got(1) == SEG_MIN and got(1 << 40) == SEG_MAX
    prev = 0
    for n in (0, 1, SEG_MIN, t256 // 2, t256 - 1, t256, t256 + 1, (t256 + t512) // 2, t512 - 1, t512, t512 + 1, 1 << 33, 1 << 40):
        v = got(n)
        assert v == seg_bytes_for(n, cus) and SEG_MIN <= v <= SEG_MAX and v >= prev, (n, cus)
        prev = v


def test_bound_is_one_rule(driver):
    for n in (0, 1, 131071, 131072, 131073, 262144, 262145, 1 << 20, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 40) + 7):
        assert [int(v) for v in driver("bound", n)[0].split()] == [bound(n), bound(n)], n
    assert bound(0) == 1048 and bound(1) == 1049 and bound(131072) == 131072 + 16384 + 1032 + 16 and bound(131073) == 131073 + 16384 + 2064 + 16


# ---- the table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", (0, 1, 2))
@pytest.mark.parametrize("shared", (0, 1, 32768))
def test_table_field_for_field(driver, shared, rule):
    jobs = job_list(IN_LENS, DICT_LENS, shared)
    cap_one = (1 << 33) + 5
    counts, totals, segs, blks = planned(driver, jobs, SEG_MIN, shared, rule, cap_one)
    want_segs, want_blks, want_totals = model(jobs, SEG_MIN, shared, rule, cap_one)
    assert segs == want_segs
    assert blks == want_blks
    assert totals == [len(want_blks)] + list(want_totals)
    nseg, max_blk = len(want_segs), len(want_segs) * MAX_SUB
    seg_tab = (nseg * SEG_JOB + 255) & ~255
    assert counts == [nseg, max_blk, seg_tab, seg_tab + max_blk * BLK_JOB, 16 * len(jobs), (max_blk + 3) & ~3,
                      4 * max_blk + 64 + 4 * nseg * MAX_SUB * HIST, 8 * (2 * max_blk + 2 + 2 * len(jobs))]
    assert totals[0] <= max_blk


@pytest.mark.parametrize("seg_bytes", (SEG_MIN, 2 * SEG_MIN, SEG_MAX))
@pytest.mark.parametrize("shared", (0, 1, 32768))
def test_table_properties(driver, shared, seg_bytes):
    """the same table held to what the kernels rely on, stated without the model"""
    jobs = job_list(IN_LENS + (SEG_MAX + 1, 3 * SEG_MAX), DICT_LENS, shared)
    counts, totals, segs, blks = planned(driver, jobs, seg_bytes, shared, 0, 0)
    assert totals[0] == len(blks) <= counts[1] and counts[0] == len(segs)
    by_seg = {}
    for i, q in enumerate(blks):
        by_seg.setdefault(q["hist_idx"] // MAX_SUB, []).append((i, q))
    k = 0
    slot = bm = d16 = 0
    for s, j in enumerate(jobs):
        dict_len = shared or j.dict_len
        pos, mine = dict_len, []
        while True:                                                          # segments tile the stream exactly
            g = segs[k]
            assert g["seg_start"] == pos and g["in"] == j.in_ptr - dict_len
            assert g["seg_end"] == min(pos + seg_bytes, dict_len + j.in_len)
            assert (g["bm_off"], g["d16_off"]) == (bm, d16)                  # scratch back to back: no two segments overlap
            bm, d16 = bm + bm_words(g["seg_end"] - pos), d16 + d16_entries(g["seg_end"] - pos)
            first, at = pos - pos % BATCH, pos
            for sub, (i, q) in enumerate(by_seg[k]):                         # blocks tile the segment in order
                assert q["blo"] == at and (q["bhi"] > at or j.in_len == 0)
                assert q["bhi"] == g["seg_end"] or (q["bhi"] - first) % SUB == 0 and q["bhi"] == first + (sub + 1) * SUB
                assert (q["hist_idx"], q["hist_prev"]) == (k * MAX_SUB + sub, int(sub > 0)) and sub < MAX_SUB
                assert (q["seg_start"], q["seg_end"], q["bm_off"], q["d16_off"], q["in"]) == (pos, g["seg_end"], g["bm_off"], g["d16_off"], g["in"])
                assert q["out"] == slot and q["out"] % 4 == 0 and q["out_cap"] == slot_bytes(q["bhi"] - q["blo"] + 258)
                slot += q["out_cap"]
                at = q["bhi"]
                mine.append(i)
            assert at == g["seg_end"]
            pos, k = g["seg_end"], k + 1
            if pos >= dict_len + j.in_len:
                break
        assert pos == dict_len + j.in_len and mine == list(range(mine[0], mine[0] + len(mine)))
        if j.in_len == 0:
            assert len(mine) == 1                                            # an empty stream: exactly one block
        for i in mine:
            q = blks[i]
            assert q["first_seg"] == mine[0] and q["stream"] & ~LAST == s and q["dst"] == j.out_ptr and q["dst_cap"] == j.out_cap
            assert bool(q["stream"] & LAST) == (i == mine[-1])
            assert q["is_last"] == int(i == mine[-1] and not j.flags & NOT_FINAL)
    assert k == len(segs) and totals[1:] == [slot, bm, d16]


def test_dst_cap_rule(driver):
    jobs = [Job(1 << 20, 1 << 30, 300000, 111, 0, 0), Job(1 << 21, 1 << 31, 5, 222, 7, 0)]
    for rule, want in ((0, [111, 222]), (1, [1 << 34, 222]), (2, [(1 << 64) - 1] * 2)):
        _, _, _, blks = planned(driver, jobs, SEG_MIN, 0, rule, 1 << 34)
        assert [sorted({q["dst_cap"] for q in blks if q["stream"] & ~LAST == s}) for s in (0, 1)] == [[w] for w in want], rule


# ---- the checks ------------------------------------------------------------------------------------------------------------------------
GOOD = dict(entry=0, level=6, strategy=0, wbits=15, null_args=0, inp=4096, out=8192, in_len=1000, dict_len=0, flags=0, out_cap=bound(1000))
TOO_LONG = (1 << 32) - SEG_MAX

ONE_CASES = [
    # (what changes, block, async)
    ({}, OK, OK),
    ({"level": 0}, OK, EINVAL), ({"level": 1}, OK, OK), ({"level": 9}, OK, OK), ({"level": 10}, EINVAL, EINVAL), ({"level": -1}, EINVAL, EINVAL),
    ({"null_args": 1}, EINVAL, EINVAL), ({"out": 0}, EINVAL, EINVAL), ({"inp": 0}, EINVAL, EINVAL),
    ({"inp": 0, "in_len": 0, "out_cap": bound(0)}, OK, OK),
    ({"inp": 0, "in_len": 0, "dict_len": 5, "out_cap": bound(0)}, OK, OK),      # (only the streams call asks for `in` here)
    ({"dict_len": 32768}, OK, OK), ({"dict_len": 32769}, EINVAL, EINVAL),
    ({"flags": NOT_FINAL | SYNC}, OK, OK), ({"flags": 4}, EINVAL, EINVAL), ({"flags": 0x80000001}, EINVAL, EINVAL),
    ({"in_len": TOO_LONG - 1, "out_cap": 1 << 40}, OK, OK), ({"in_len": TOO_LONG, "out_cap": 1 << 40}, EINVAL, EINVAL),
    ({"in_len": TOO_LONG - 32768, "dict_len": 32768, "out_cap": 1 << 40}, EINVAL, EINVAL),
    ({"in_len": 1 << 33, "out_cap": 1 << 40}, EINVAL, EINVAL),
    ({"out_cap": bound(1000) - 1}, BUF, BUF), ({"out_cap": 0}, BUF, BUF),
    # every ZNG_ROCM_EINVAL comes before -5
    ({"out_cap": 0, "level": 10}, EINVAL, EINVAL), ({"out_cap": 0, "dict_len": 40000}, EINVAL, EINVAL), ({"out_cap": 0, "flags": 8}, EINVAL, EINVAL),
    ({"out_cap": 0, "null_args": 1}, EINVAL, EINVAL), ({"out_cap": 0, "in_len": TOO_LONG}, EINVAL, EINVAL),
]
BLOCK_ONLY = [({"strategy": 4}, OK), ({"strategy": 5}, EINVAL), ({"strategy": -1}, EINVAL), ({"wbits": 9}, OK), ({"wbits": 8}, EINVAL),
              ({"wbits": 16}, EINVAL), ({"wbits": 0}, EINVAL), ({"out_cap": 0, "strategy": 5}, EINVAL), ({"out_cap": 0, "wbits": 8}, EINVAL),
              ({"level": 0, "strategy": 3, "wbits": 9}, OK)]


def _one(driver, entry, change):
    a = dict(GOOD, entry=entry, **change)
    return int(driver("one", a["entry"], a["level"], a["strategy"], a["wbits"], a["null_args"], a["inp"], a["out"], a["in_len"],
                      a["dict_len"], a["flags"], a["out_cap"])[0])


def test_checks_of_the_one_stream_calls(driver):
    for change, block, asyn in ONE_CASES:
        assert _one(driver, 0, change) == block, ("block", change)
        assert _one(driver, 1, change) == asyn, ("async", change)
    for change, block in BLOCK_ONLY:
        assert _one(driver, 0, change) == block, ("block", change)


def _streams(driver, jobs, level=6, strategy=0, wbits=15, null_jobs=0, null_out_lens=0):
    status, bad = (int(v) for v in driver("streams", level, strategy, wbits, null_jobs, null_out_lens, *[v for j in jobs for v in j.args])[0].split())
    return status, bad


def test_checks_of_the_streams_call(driver):
    def good(n=1000, **kw):
        a = dict(in_ptr=4096, out_ptr=8192, in_len=n, out_cap=bound(n), dict_len=0, flags=0)
        a.update(kw)
        return Job(**a)
    three = [good(), good(5), good(0)]
    assert _streams(driver, three) == (OK, 3)
    for level, want in ((0, EINVAL), (1, OK), (9, OK), (10, EINVAL)):
        assert _streams(driver, three, level=level)[0] == want, level
    for strategy, want in ((-1, EINVAL), (4, OK), (5, EINVAL)):
        assert _streams(driver, three, strategy=strategy)[0] == want, strategy
    for wbits, want in ((8, EINVAL), (9, OK), (14, OK), (16, EINVAL)):
        assert _streams(driver, three, wbits=wbits)[0] == want, wbits
    assert _streams(driver, three, null_jobs=1)[0] == EINVAL and _streams(driver, three, null_out_lens=1)[0] == EINVAL
    # a call without jobs: taken once strategy and window are in range -- before the level and the pointers are looked at
    assert _streams(driver, [], level=0, null_jobs=1, null_out_lens=1) == (OK, 0)
    assert _streams(driver, [], level=77) == (OK, 0)
    assert _streams(driver, [], strategy=5)[0] == EINVAL and _streams(driver, [], wbits=8)[0] == EINVAL
    # one job
    for kw, want in (({"out_ptr": 0}, EINVAL), ({"in_ptr": 0}, EINVAL), ({"in_ptr": 0, "in_len": 0, "out_cap": bound(0)}, OK),
                     ({"in_ptr": 0, "in_len": 0, "out_cap": bound(0), "dict_len": 5}, EINVAL), ({"dict_len": 32768}, OK),
                     ({"dict_len": 32769}, EINVAL), ({"flags": 3}, OK), ({"flags": 4}, EINVAL), ({"out_cap": bound(1000) - 1}, BUF),
                     ({"in_len": TOO_LONG - 1, "out_cap": 0xffffffff}, BUF), ({"in_len": TOO_LONG, "out_cap": 0xffffffff}, EINVAL),
                     ({"in_len": TOO_LONG - 5, "dict_len": 5, "out_cap": 0xffffffff}, EINVAL), ({"out_cap": 0, "flags": 4}, EINVAL)):
        assert _streams(driver, [good(), good(**kw), good()]) == (want, 1 if want else 3), kw
    # the first refusal in job order: a short buffer in front of a bad argument is -5, behind it ZNG_ROCM_EINVAL
    assert _streams(driver, [good(), good(out_cap=0), good(flags=4)]) == (BUF, 1)
    assert _streams(driver, [good(flags=4), good(out_cap=0)]) == (EINVAL, 0)
    # the call's own refusals come before any job's
    assert _streams(driver, [good(out_cap=0)], level=0) == (EINVAL, 1)
    assert _streams(driver, [good(out_cap=0)], strategy=9) == (EINVAL, 1)


# ---- the round cut ---------------------------------------------------------------------------------------------------------------------
def _round_model(jobs, first, room, count_dict):
    last, total = first, 0
    while last < len(jobs):
        n = jobs[last].in_len + (jobs[last].dict_len if count_dict else 0)
        if last > first and total + n > room:
            break
        total, last = total + n, last + 1
    return last


def test_round_cut(driver):
    jobs = [Job(4096, 8192, n, 0, d, 0) for n, d in ((100, 0), (50, 50), (100, 1), (1000, 0), (0, 0), (0, 10), (99, 1), (1, 0), (100, 100))]
    for room in (1, 99, 100, 101, 200, 201, 250, 301, 1 << 20):
        for first in range(len(jobs) + 1):
            for count_dict in (0, 1):
                got = [int(v) for v in driver("round", count_dict, room, first, *[v for j in jobs for v in j.args])[0].split()]
                want = _round_model(jobs, first, room, count_dict)
                assert got == [want] * (1 if count_dict else 2), (room, first, count_dict)          # (cs_round_end: the same cut)
                assert want > first or first == len(jobs)
    # the two ways of counting differ, and a job longer than a round still gets a round of its own
    assert _round_model(jobs, 0, 200, 0) == 2 and _round_model(jobs, 0, 200, 1) == 2 and _round_model(jobs, 1, 200, 0) == 3
    assert _round_model(jobs, 1, 200, 1) == 2 and _round_model(jobs, 3, 100, 1) == 4 and _round_model(jobs, 3, 100, 0) == 4
    big = [Job(4096, 8192, 0xfff00000, 0, 0, 0), Job(4096, 8192, 0xfff00000, 0, 32768, 0), Job(4096, 8192, 10, 0, 0, 0)]
    for count_dict in (0, 1):
        ends = [int(driver("round", count_dict, 4 << 30, f, *[v for j in big for v in j.args])[0].split()[0]) for f in range(3)]
        assert ends == [1, 3, 3], count_dict


# ---- the sweep -----------------------------------------------------------------------------------------------------------------------
def test_no_block_without_positions(driver):
    """What the block cut once had a branch for -- a block [blo, bhi) with blo >= bhi in a stream that has plaintext -- does not
    occur: first <= a < first + 61440 and the last block begins below b.  The model, over every dict_len mod 1024 and every
    in_len around a border; then the planner itself over the same grid (and both segment sizes)."""
    skipped = cases = 0
    for d in range(1024):
        lens = {0, 1, 2, 3 * SUB + 2}
        for k in (1, 2, 3):
            for e in (-1, 0, 1):
                lens |= {k * SUB + e, k * SUB - d + e, k * SUB - d - BATCH + e}
        for n in lens:
            a, b = d, d + n
            first = a - a % BATCH
            nsub = -(-(b - first) // SUB) if b > first else 1
            for sub in range(nsub):
                p0 = first + sub * SUB
                blo, bhi = max(p0, a), min(p0 + SUB, b)
                skipped += blo >= bhi and not (b == a and sub + 1 == nsub)
            cases += 1
    print("model: %d cases, %d blocks without positions" % (cases, skipped))
    assert skipped == 0
    got_cases, blocks, empty = (int(v) for v in driver("sweep")[0].split())
    print("planner: %d cases, %d blocks, %d without positions" % (got_cases, blocks, empty))
    assert got_cases >= 1024 * 25 and blocks > got_cases and empty == 0


def test_self_check(driver):
    assert driver("self") == ["self ok"]
