"""CPU checks of the host side of BGZF random access (zng_rocm_bgzf_index_dev, zng_rocm_bgzf_read_dev, zng_rocm_bgzf_voffset /
_uoffset): the rules of zlib-ng_amd/csrc/bgzf_read_plan.h through a small C++ driver (tests/c/bgzf_read_plan_driver.cpp) built
here with g++ -Wall -Wextra -Werror.

  the chain walk   from offset 0 along BSIZE; candidates inside a member are never looked at; behind a complete member fewer
                   than two bytes or two bytes other than 1f 8b are garbage (0), 1f 8b has to be a BGZF member (-3), a BSIZE end
                   behind the file or a header the file's end cuts is -5
  the row check    ascending and not overlapping, inside src_len, dst_off contiguous from 0, bgzf 1, 28 <= src_len <= 65536,
                   out_len <= 65536
  the plan         clipping at plain_len; a member wholly inside a range is interior (a job of its own, straight to the
                   destination), a member that is cut is an edge: one job per round however many ranges cut it, and a slice per
                   range; a round ends in front of the range whose new edges find no slot
  the results      the verdict on a job, the worst failure of a range, the bytes in front of the first failing part
  virtual offsets  src_off << 16 | offset in the member; a member's end is offset 0 of the next non-empty member
Every expected value is worked out here from these rules."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BGZF, CUT, INSIDE, ROOM, TRAILER, NEXT_MAGIC = 1, 2, 4, 8, 16, 32
NO_HEADER, NO_ROOM, ISIZE, CUT_HEADER, CUT_MEMBER = 1, 2, 3, 4, 5
ORDER, OUTSIDE, DST_OFF, NOT_BGZF, SRC_LEN, OUT_LEN = 1, 2, 3, 4, 5, 6
DIRECT = 0xffffffff
MSG_ROW = 0xffffffff
LOOK = 4096


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "bgzf_read_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-O1",
                               "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"),
                               os.path.join(ROOT, "tests", "c", "bgzf_read_plan_driver.cpp"), "-o", exe])

        def run(cmd, *numbers):
            flat = []
            for v in numbers:
                flat.extend(v if isinstance(v, (list, tuple)) else [v])
            out = subprocess.run([exe, cmd], input=" ".join(str(int(v)) for v in flat), capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, (cmd, out.returncode, out.stderr)
            return [[int(x) if x.lstrip("-").isdigit() else x for x in line.split()] for line in out.stdout.splitlines()]
        yield run


# ---- the chain walk ---------------------------------------------------------------------------------------------------------
def flags(bgzf, cut, pos, end, header_len, src_len, next_magic=False):
    f = CUT if cut else 0
    if bgzf:
        f |= BGZF
        inside, room = end <= src_len, end - pos >= header_len + 10
        f |= (INSIDE if inside else 0) | (ROOM if room else 0) | (TRAILER if inside and room else 0)
    return f | (NEXT_MAGIC if next_magic else 0)


def member_row(pos, size, isize, crc, src_len, next_magic, header_len=18):
    return (pos, pos + size, header_len, crc, isize, flags(True, False, pos, pos + size, header_len, src_len, next_magic))


def other_row(pos, src_len, cut=False):
    """a candidate that is no BGZF member: a plain gzip header, a refused one, or (cut) one the header kernel ran out of"""
    return (pos, pos, 0, 0, 0, flags(False, cut, pos, pos, 0, src_len))


def walk(driver, src_len, rows, cap=64, look=LOOK):
    out = driver("walk", src_len, look, cap, len(rows), *rows)
    return tuple(out[0]), [tuple(r) for r in out[1:]]


def test_index_flags(driver):
    for bgzf, cut, pos, end, hl, n in ((1, 0, 0, 28, 18, 28), (1, 0, 0, 28, 18, 27), (1, 0, 5, 32, 18, 100), (1, 0, 5, 33, 18, 100),
                                       (1, 0, 0, 40, 30, 40), (1, 0, 0, 39, 30, 39), (0, 0, 7, 7, 0, 100), (0, 1, 7, 7, 0, 100),
                                       (1, 0, 0, 65536, 18, 65536), (1, 0, 0, 1, 18, 100)):
        assert driver("flags", bgzf, cut, pos, end, hl, n) == [[flags(bgzf, cut, pos, end, hl, n)]], (bgzf, cut, pos, end, hl, n)
    assert flags(1, 0, 0, 28, 18, 28) == BGZF | INSIDE | ROOM | TRAILER and flags(1, 0, 5, 32, 18, 100) == BGZF | INSIDE


def clean(sizes, isizes, tail=0):
    """rows of a clean file: members of `sizes` bytes one behind the other, `tail` bytes behind them"""
    src_len = sum(sizes) + tail
    rows, want, at, out = [], [], 0, 0
    for k, (size, isize) in enumerate(zip(sizes, isizes)):
        rows.append(member_row(at, size, isize, 0x1000 + k, src_len, k + 1 < len(sizes)))
        want.append((at, size, out, isize, 0x1000 + k, 1))
        at += size
        out += isize
    return src_len, rows, want


def test_walk_clean_file_and_members_cap(driver):
    src_len, rows, want = clean([100, 65536, 28, 300, 28], [500, 65536, 0, 65280, 0])
    head, got = walk(driver, src_len, rows)
    assert head == (0, 0, src_len, 500 + 65536 + 65280, 5) and got == want
    for cap in (0, 1, 4, 5):
        head, got = walk(driver, src_len, rows, cap=cap)
        assert head == (0, 0, src_len, 500 + 65536 + 65280, 5) and got == want[:cap], cap


def test_walk_hops_over_candidates_inside_a_member(driver):
    src_len, rows, want = clean([100, 200, 28], [500, 600, 0])
    # inside member 0: a plain header, a cut one and a would-be BGZF member whose end lies behind the file; inside member 1:
    # a BGZF candidate that ends exactly where member 1 ends
    inside = [other_row(10, src_len), other_row(50, src_len, cut=True), member_row(60, 5000, 7, 7, src_len, False),
              member_row(150, 150, 9, 9, src_len, True)]
    rows = sorted(rows + inside)
    head, got = walk(driver, src_len, rows)
    assert head == (0, 0, src_len, 1100, 3) and got == want


@pytest.mark.parametrize("tail", [0, 1, 2, 3, 4, 40])
def test_walk_trailing_garbage(driver, tail):
    src_len, rows, want = clean([100, 28], [500, 0], tail=tail)
    head, got = walk(driver, src_len, rows)                    # two bytes other than 1f 8b, or fewer than two
    assert head == (0, 0, 128, 500, 2) and got == want
    # 1f 8b behind the last member: one byte of it is garbage (gz_look asks avail_in > 1); two and more have to be a member
    rows[-1] = member_row(100, 28, 0, 0x1001, src_len, tail >= 2)
    head, got = walk(driver, src_len, rows)
    # (1f 8b and fewer than two bytes behind it: a header the file's end cuts)
    assert head == ((0, 0, 128, 500, 2) if tail < 2 else (-5, CUT_HEADER, 128, 500, 2) if tail < 4 else (-3, NO_HEADER, 128, 500, 2))
    assert got == want


def test_walk_non_bgzf_member_behind_a_complete_one(driver):
    src_len, rows, want = clean([100, 100], [500, 600], tail=50)
    rows[-1] = member_row(100, 100, 600, 0x1001, src_len, True)
    for third in (other_row(200, src_len),                                  # a plain gzip member, or a refused header
                  other_row(200, 200 + LOOK + 1, cut=True),                 # a header longer than the kernel is shown: refused
                  member_row(200, 25, 0, 0, src_len, False),                # BSIZE leaves no room
                  member_row(200, 50, 65537, 0, src_len, False)):           # ISIZE above 65536
        n = 200 + LOOK + 1 if third[5] & CUT else src_len
        head, got = walk(driver, n, rows + [third])
        why = NO_ROOM if third[1] == 225 else ISIZE if third[4] == 65537 else NO_HEADER
        assert head == (-3, why, 200, 1100, 2) and got == want, third
    head, got = walk(driver, src_len, rows)                                 # 1f 8b 09: no candidate at all
    assert head == (-3, NO_HEADER, 200, 1100, 2) and got == want
    ok = member_row(200, 50, 65536, 5, src_len, False)                      # ISIZE of exactly 65536 is a member
    assert walk(driver, src_len, rows + [ok])[0] == (0, 0, 250, 1100 + 65536, 3)


def test_walk_truncated(driver):
    src_len, rows, want = clean([100, 100], [500, 600])
    rows[-1] = member_row(100, 100, 600, 0x1001, 199, False)                # BSIZE end one byte behind the file
    head, got = walk(driver, 199, rows)
    assert head == (-5, CUT_MEMBER, 100, 500, 1) and got == want[:1]
    rows[-1] = other_row(100, 110, cut=True)                                # the file ends inside the header
    head, got = walk(driver, 110, rows)
    assert head == (-5, CUT_HEADER, 100, 500, 1) and got == want[:1]
    rows[0] = member_row(0, 100, 500, 0x1000, 110, True)
    assert walk(driver, 110, rows)[0] == (-5, CUT_HEADER, 100, 500, 1)


def test_walk_empty_and_offset_zero(driver):
    assert walk(driver, 0, []) == ((0, 0, 0, 0, 0), [])
    for n in (1, 3, 17):                                                    # shorter than a BGZF header
        assert walk(driver, n, [])[0] == (-5, CUT_HEADER, 0, 0, 0)
    assert walk(driver, 18, [])[0] == (-3, NO_HEADER, 0, 0, 0)              # garbage from the first byte
    assert walk(driver, 500, [other_row(0, 500)])[0] == (-3, NO_HEADER, 0, 0, 0)          # a plain gzip file
    assert walk(driver, 500, [other_row(7, 500)])[0] == (-3, NO_HEADER, 0, 0, 0)
    assert walk(driver, 12, [other_row(0, 12, cut=True)])[0] == (-5, CUT_HEADER, 0, 0, 0)


# ---- the row check ----------------------------------------------------------------------------------------------------------
TABLE_OUT = [5, 3, 0, 4, 1, 6, 2, 0]                                       # an empty member in the middle, the end-of-file row


def table(out_lens=TABLE_OUT, gap=0):
    rows, at, out = [], 0, 0
    for k, n in enumerate(out_lens):
        size = 28 + n
        rows.append([at, size, out, n, 0x2000 + k, 1])
        at += size + gap
        out += n
    return rows, at - gap


def test_row_check(driver):
    rows, src_len = table()
    assert driver("check", src_len, len(rows), *rows) == [[0, len(rows)]]
    assert driver("check", 0, 0) == [[0, 0]]
    gapped, gl = table(gap=3)                                               # bytes between members are not refused
    assert driver("check", gl, len(gapped), *gapped) == [[0, len(gapped)]]

    def refused(why, k, edit, n=src_len):
        bad = [list(r) for r in rows]
        edit(bad)
        assert driver("check", n, len(bad), *bad) == [[why, k]], (why, k)
    refused(OUTSIDE, 7, lambda t: None, n=src_len - 1)
    refused(ORDER, 3, lambda t: t[3].__setitem__(0, t[3][0] - 1))           # overlaps the member in front
    refused(ORDER, 2, lambda t: (t[2].__setitem__(0, t[1][0])))             # the same offset twice
    refused(DST_OFF, 0, lambda t: t[0].__setitem__(2, 1))                   # not from 0
    refused(DST_OFF, 4, lambda t: t[4].__setitem__(2, t[4][2] + 1))
    refused(DST_OFF, 4, lambda t: t[3].__setitem__(3, t[3][3] - 1))         # a shorter member in front: the next dst_off is off
    refused(NOT_BGZF, 5, lambda t: t[5].__setitem__(5, 0))
    refused(NOT_BGZF, 5, lambda t: t[5].__setitem__(5, 2))
    refused(SRC_LEN, 6, lambda t: t[6].__setitem__(1, 27))
    refused(SRC_LEN, 6, lambda t: t[6].__setitem__(1, 65537))
    refused(OUT_LEN, 1, lambda t: t[1].__setitem__(3, 65537))
    big = [[0, 65536, 0, 65536, 1, 1], [65536, 28, 65536, 0, 0, 1]]
    assert driver("check", 65564, 2, *big) == [[0, 2]]


def test_scratch_bytes(driver):
    KiB = 1 << 10
    for scratch, want in ((0, 4096), (128 * KiB, 2), (128 * KiB - 1, 0), (1, 0), (192 * KiB, 3), (256 << 20, 4096), (4 << 30, 65536),
                          ((4 << 30) + 1, 0), (1 << 40, 0)):
        assert driver("slots", scratch) == [[want]], scratch


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def want_plan(rows, ranges, slots, round_jobs):
    """the rules restated with a linear search per range"""
    plain_len = rows[-1][2] + rows[-1][3] if rows else 0
    clipped, jobs, parts, rounds = [], [], [], []
    cur = dict(rb=0, jb=0, pb=0, slots=0, slices=0)
    edge = {}

    def close(range_end):
        if len(jobs) > cur["jb"]:
            rounds.append((cur["rb"], range_end, cur["jb"], len(jobs), cur["pb"], len(parts), cur["slots"], cur["slices"]))
        cur.update(rb=range_end, jb=len(jobs), pb=len(parts), slots=0, slices=0)
        edge.clear()

    for r, (uoff, ln) in enumerate(ranges):
        n = 0 if uoff >= plain_len else min(ln, plain_len - uoff)
        clipped.append(n)
        if not n:
            continue
        touched = [i for i, m in enumerate(rows) if m[3] and m[2] < uoff + n and m[2] + m[3] > uoff]
        whole = {i: rows[i][2] >= uoff and rows[i][2] + rows[i][3] <= uoff + n for i in touched}
        fresh = sum(1 for i in touched if not whole[i] and i not in edge)
        assert fresh <= 2 and all(whole[i] for i in touched[1:-1])
        if cur["slots"] + fresh > slots and len(jobs) > cur["jb"]:
            close(r)
        for i in touched:
            lo, hi = max(rows[i][2], uoff), min(rows[i][2] + rows[i][3], uoff + n)
            if whole[i]:
                jobs.append((i, DIRECT, r, lo - uoff))
                parts.append((r, len(jobs) - 1, lo - uoff, 0, rows[i][3], 0))
                continue
            if i not in edge:
                jobs.append((i, cur["slots"], 0, 0))
                cur["slots"] += 1
                edge[i] = len(jobs) - 1
            parts.append((r, edge[i], lo - uoff, lo - rows[i][2], hi - lo, 1))
            cur["slices"] += 1
        if len(jobs) - cur["jb"] >= round_jobs:
            close(r + 1)
    close(len(ranges))
    direct = sum(1 for j in jobs if j[1] == DIRECT)
    return clipped, jobs, parts, rounds, len(jobs), direct


def run_plan(driver, rows, ranges, slots=4096, round_jobs=1 << 22):
    out = driver("plan", slots, round_jobs, len(rows), len(ranges), *rows, *ranges)
    decoded, direct, nj, np_, nr = out[0]
    clipped = out[1]
    lines = out[2:]
    jobs = [tuple(x[1:]) for x in lines if x[0] == "J"]
    parts = [tuple(x[1:]) for x in lines if x[0] == "P"]
    rounds = [tuple(x[1:]) for x in lines if x[0] == "R"]
    assert (nj, np_, nr) == (len(jobs), len(parts), len(rounds))
    return clipped, jobs, parts, rounds, decoded, direct


def deliver(rows, plain, ranges, plan):
    """what the plan writes: per range the bytes its parts put into its destination"""
    clipped, jobs, parts = plan[0], plan[1], plan[2]
    dst = [bytearray(b"\xab" * n) for n in clipped]
    for r, job, at, off, ln, is_slice in parts:
        member, slot, jr, jat = jobs[job]
        text = plain[rows[member][2]:rows[member][2] + rows[member][3]]
        assert (slot != DIRECT) == bool(is_slice)
        if not is_slice:
            assert (jr, jat, off, ln) == (r, at, 0, len(text))
        dst[r][at:at + ln] = text[off:off + ln]
    return [bytes(d) for d in dst]


def test_plan_classes_slices_and_sharing(driver):
    rows, _ = table()                                                       # plaintext 0..21: 5 | 3 | - | 4 | 1 | 6 | 2 | -
    ranges = [(6, 1),        # inside member 1: one edge
              (5, 3),        # exactly member 1: interior
              (3, 14),       # edge 0, interiors 1 3 4, edge 5 (the empty member 2 is skipped)
              (7, 100),      # edge 1 (shared with range 0), interiors 3 4 5 6, clipped at 21
              (21, 5),       # uoff == plain_len
              (30, 5),       # beyond
              (4, 0),        # len 0
              (4, 2)]        # edges 0 (shared with range 2) and 1
    got = run_plan(driver, rows, ranges)
    assert got == want_plan(rows, ranges, 4096, 1 << 22)
    clipped, jobs, parts, rounds, decoded, direct = got
    assert clipped == [1, 3, 14, 14, 0, 0, 0, 2]
    assert [j[0] for j in jobs] == [1, 1, 0, 1, 3, 4, 5, 3, 4, 5, 6]        # edge 1 once, edge 0 once, edge 5 once
    assert [j[1] for j in jobs] == [0, DIRECT, 1, DIRECT, DIRECT, DIRECT, 2, DIRECT, DIRECT, DIRECT, DIRECT]
    assert (decoded, direct) == (11, 8) and rounds == [(0, 8, 0, 11, 0, len(parts), 3, 6)]
    slices = [p for p in parts if p[5]]
    assert slices == [(0, 0, 0, 1, 1, 1), (2, 2, 0, 3, 2, 1), (2, 6, 10, 0, 4, 1), (3, 0, 0, 2, 1, 1), (7, 2, 0, 4, 1, 1), (7, 0, 1, 0, 1, 1)]
    plain = bytes(range(65, 65 + 21))
    assert deliver(rows, plain, ranges, got) == [plain[u:u + n][:c] for (u, n), c in zip(ranges, clipped)]


@pytest.mark.parametrize("slots, round_jobs", [(4096, 1 << 22), (2, 1 << 22), (3, 1 << 22), (4096, 1), (2, 4)])
def test_plan_against_brute_force(driver, slots, round_jobs):
    rows, _ = table()
    plain = bytes(range(65, 65 + 21))
    ranges = [(u, n) for u in range(0, 24) for n in range(0, 25)] + [(3, 1 << 63), (0, (1 << 64) - 1), ((1 << 64) - 1, (1 << 64) - 1)]
    got = run_plan(driver, rows, ranges, slots, round_jobs)
    assert got == want_plan(rows, ranges, slots, round_jobs)
    clipped, jobs, parts, rounds, decoded, direct = got
    assert clipped == [max(0, min(n, 21 - u)) for u, n in ranges]
    assert deliver(rows, plain, ranges, got) == [plain[u:u + n] for u, n in ranges]
    # rounds: consecutive, every range's parts in one round, no more edge slots than allowed, no edge decoded twice in a round
    assert all(a[1] <= b[0] and a[3] == b[2] and a[5] == b[4] for a, b in zip(rounds, rounds[1:]))
    assert rounds[0][2] == 0 and rounds[-1][3] == len(jobs) and rounds[-1][5] == len(parts)
    for rb, re_, jb, je, pb, pe, nslots, nslices in rounds:
        assert nslots <= slots and all(rb <= p[0] < re_ and jb <= p[1] < je for p in parts[pb:pe])
        edges = [j for j in jobs[jb:je] if j[1] != DIRECT]
        assert len({j[0] for j in edges}) == len(edges) == nslots and sorted(j[1] for j in edges) == list(range(nslots))
        assert nslices == sum(p[5] for p in parts[pb:pe])
    if slots == 2:
        assert len(rounds) > 1
    if round_jobs == 1:
        assert all(je - jb <= 6 for _, _, jb, je, *_ in rounds)             # closed behind the range that passed the bound


def test_plan_rounds_under_small_scratch(driver):
    rows, _ = table()
    ranges = [(4, 2), (4, 2), (7, 3), (4, 5), (0, 21)]                      # edges {0,1}, the same, {1,3}, {0,3} around 1, none
    clipped, jobs, parts, rounds, decoded, direct = run_plan(driver, rows, ranges, slots=2)
    assert [(r[0], r[1], r[6]) for r in rounds] == [(0, 2, 2), (2, 3, 2), (3, 5, 2)]
    assert (decoded, direct) == (2 + 2 + 3 + 6, 1 + 6)
    one = run_plan(driver, rows, ranges, slots=3)                           # every edge finds a slot: one round, each edge once
    assert [(r[0], r[1], r[6]) for r in one[3]] == [(0, 5, 3)] and (one[4], one[5]) == (3 + 1 + 6, 1 + 6)
    assert run_plan(driver, [], [(0, 5), (1, 0)])[:4] == ([0, 0], [], [], [])


# ---- results ----------------------------------------------------------------------------------------------------------------
def test_job_verdict(driver):
    v = lambda *a: tuple(driver("verdict", *a)[0])                          # noqa: E731
    assert v(500, 100, 1, 0, 100, 500) == (1, 0)
    assert v(499, 100, 1, 0, 100, 500) == (-3, MSG_ROW) and v(500, 99, 1, 0, 100, 500) == (-3, MSG_ROW)
    assert v(500, 100, -3, 9, 100, 500) == (-3, 9) and v(0, 0, -3, 4, 100, 500) == (-3, 4)
    assert v(200, 100, -5, 0, 100, 500) == (-5, 0) and v(500, 100, -5, 3, 100, 500) == (-5, 0)
    assert v(0, 28, 1, 0, 28, 0) == (1, 0)


def test_range_result(driver):
    def result(clipped, parts, verdicts):
        return tuple(driver("result", clipped, len(parts), len(verdicts), *parts, *verdicts)[0])
    parts = [(0, 0), (1, 10), (2, 30), (3, 70)]
    ok, data, row, short = (1, 0), (-3, 6), (-3, MSG_ROW), (-5, 0)
    assert result(90, parts, [ok, ok, ok, ok]) == (1, 90, 0, 0)
    assert result(0, [], []) == (1, 0, 0, 0)
    assert result(90, parts, [ok, data, ok, ok]) == (-3, 10, 1, 6)
    assert result(90, parts, [data, ok, ok, ok]) == (-3, 0, 1, 6)
    assert result(90, parts, [ok, ok, ok, short]) == (-5, 70, 0, 0)
    assert result(90, parts, [ok, short, row, ok]) == (-3, 10, 1, MSG_ROW)   # -3 outweighs -5; out_len from the first failure
    assert result(90, parts, [ok, ok, row, data]) == (-3, 30, 1, MSG_ROW)    # the first -3's message
    assert result(90, [(5, 0), (2, 40)], [ok, ok, short, ok, ok, ok]) == (-5, 40, 0, 0)


# ---- virtual offsets --------------------------------------------------------------------------------------------------------
def test_virtual_offsets(driver):
    rows, _ = table()
    uoffs = list(range(0, 23))
    got = [x[0] for x in driver("voff", len(rows), len(uoffs), *rows, *uoffs)]
    want = []
    for u in uoffs:
        holder = [m for m in rows if m[2] <= u < m[2] + m[3]]
        m = holder[0] if holder else rows[-1]
        want.append((m[0] << 16) | (u - m[2]) if u <= 21 else "refused")
    assert got == want
    assert got[5] == rows[1][0] << 16 and got[8] == rows[3][0] << 16        # a member's end: offset 0 of the next non-empty one
    assert got[21] == rows[7][0] << 16                                      # plain_len: the start of the last row
    back = [x[0] for x in driver("uoff", len(rows), 22, *rows, *got[:22])]
    assert back == uoffs[:22]
    # the inverse also takes the offset AT a member's end, and an empty member's start
    ask = [(rows[0][0] << 16) | 5, rows[2][0] << 16, (rows[2][0] << 16) | 1, (rows[0][0] << 16) | 6, (rows[0][0] + 1) << 16,
           (rows[7][0] << 16) | 1, (1 << 64) - 1]
    assert [x[0] for x in driver("uoff", len(rows), len(ask), *rows, *ask)] == [5, 8, "refused", "refused", "refused", "refused", "refused"]
    assert driver("voff", 0, 1, 0) == [["refused"]] and driver("uoff", 0, 1, 0) == [["refused"]]
    far = [[1 << 48, 40, 0, 12, 1, 1]]                                      # src_off does not fit 48 bits
    assert driver("voff", 1, 1, *far, 3) == [["refused"]]
    near = [[(1 << 48) - 1, 40, 0, 12, 1, 1]]
    assert driver("voff", 1, 2, *near, 3, 12) == [[(((1 << 48) - 1) << 16) | 3], [(((1 << 48) - 1) << 16) | 12]]
    full = [[0, 65536, 0, 65536, 1, 1]]                                     # plain_len behind a last row of 65536 bytes
    assert driver("voff", 1, 2, *full, 65535, 65536) == [[65535], ["refused"]]

