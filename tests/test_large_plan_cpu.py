"""CPU checks of the host plan of the large inflater (zlib-ng_amd/csrc/inflate_large_plan.h): the chain walk over the parts'
result words and the grouping of parts into segments, which the one-stream call and the batch share.  A small C++ driver
(tests/c/large_plan_driver.cpp) is built here with g++ and fed hand-written tables; every expected value below is worked out
by hand from the rules in the header's and the part kernel's comments:

  result words of a part  r = [symbols, end bit lo, end bit hi, 1 = ended the BFINAL block, message, reach, link, -]
  side words (SUBBLOCK)   s = [symbols of the first block or NONE, its end bit lo, hi, its reach, handed off inside a block,
                               that block's BFINAL (2 = unknown), -, -]
  marks (blocks mode)     m = [symbols of the complete blocks, their end bit lo, hi, their reach]

  part 0 is genuine; the part a genuine part links to is genuine; nothing else is.  A link points forward and into its own
  stream.  A reach may not pass the bytes in front of the part (produced + window_len).  A key-1 part that begins inside the
  BFINAL block ends the stream where its first block ended.  Segments are closed at >= 40960 symbols; a last one below 32768
  joins the one in front of it unless it is the only one.

The rules the device pass reads its scratch and its second launch from are driven the same way (the driver's `layout`, `retry`
and `segs` arguments), and so are the finder's host rules (`finder`):

  finder       a pass over N streams is cut into work items of a 4096th of its bytes, a multiple of 4096 within 4 .. 64 KiB;
               room for a survivor per 64 bytes (F1) and per 512 (F2, the patterns) and 4096 per stream; a survivor goes to
               the stream its tag (bits 40-61) names, without the tag and bit 63, and each stream's list is sorted by bit
  part tables jobs (40 bytes per part) | starts (8; SUBBLOCK: | keys, 8) | results (8 words; blocks mode: | marks, 4 words;
               SUBBLOCK: | side words, 8 words) | slots, every table at a multiple of 256 bytes; the pinned mirror ends where
               the slots begin
  retry        a part that said "output full" (message 13) runs again with retry_cap = (1032 x its compressed bytes + 655360,
               rounded up to 8) symbols of room, the parts one behind the other; a stream whose parts want more than the
               limit in bytes (2 per symbol) is reported and left out
  chainfull    a piece over that limit runs the full parts ON its chain again, one at a time: the first full part that following
               the links from the stream's first part meets, "end" when the chain ends without one, "broken" otherwise
  symbol array streams one behind the other, each behind a gap of 32768 symbols, the first at 32768; a copy's dst is re-based
               to the array, gstart / first name the first copy of its segment; a segment's bytes end where the next segment
               of the same stream begins, the last one's where the stream's do

And the rules the pieces loop steps by (`pieces`; tools/sanitize_inflate_large_plan.sh runs the driver's `self` sweep of them
under ASan + UBSan):

  next piece   [bit >> 3, end): p bytes, the stream's end when that is nearer, and a quarter of p in front of the stream's end
               when less than a quarter would be left; the pass's buffer begins at base = the piece's first byte -- the byte
               of the dynamic header H, for a key of H + 2 with H in front -- rounded down to 256; the pass counts bits from
               there: start_bit = bit - 8 base, scan_lo = (bit >> 3) - base, key0 = key - 8 base for a key of 2 and more
  after a pass not stopped: done, in_used = base + used.  Stopped: bit and a key of 2 and more go back by + 8 base, fin is the
               chain's, p is piece_bytes again, and a key of 0 moves the anchor (abit, aout) to (bit, produced)
  halving      to p / 2 while that is at least 4 MiB (kPieceMin)
  history      the last min(32768, pos + window_len) bytes in front of output position pos: in the output when pos has them
               all; the window as it stands at pos 0; else the window's last (that - pos) bytes and then the pos delivered
  sequential   from byte a0 = abit >> 3, bit sb = abit & 7: max(2 p, (bit >> 3) - a0 + p) bytes, doubled while the blocks form
               says 0 with its end bit still sb and input is left; its answer stands on 1, on 0 with the end bit moved and on
               -4, anything else is decoded again in the stream form; behind complete blocks up to bit eb the state is
               bit = 8 a0 + eb, key 0, fin -1, the anchor there, p = piece_bytes"""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = 0xFFFFFFFF
STARVED, LITLEN_CODE, OUT_FULL = 12, 9, 13        # InflateMsg: kMsgStarved, kMsgLitLenCode, kMsgOutFull
NO_SIDE = [NONE, 0, 0, 0, 0, 0, 0, 0]


@pytest.fixture(scope="module")
def driver():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "large_plan_driver")
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1",
                               "-I" + os.path.join(ROOT, "zlib-ng_amd", "csrc"),
                               os.path.join(ROOT, "tests", "c", "large_plan_driver.cpp"), "-o", exe])
        yield exe


def part(n, end, ended=0, msg=0, reach=0, link=NONE):
    return [n, end & 0xFFFFFFFF, end >> 32, ended, msg, reach, link, 0]


def walk(exe, starts, res, keys=None, side=None, marks=None, pbase=0, window_len=0, src_len=1000, sub=0, blocks=0):
    """-> (status line, produced, end_bit, final, subparts, [(table row, dst, n)], seg_first)"""
    rows, np_ = len(res), len(starts)
    keys = keys or [0] * np_
    side = side or [NO_SIDE] * rows
    marks = marks or [[0, 0, 0, 0]] * rows
    assert len(keys) == np_ and len(side) == rows and len(marks) == rows and pbase + np_ <= rows
    words = [rows, pbase, np_, window_len, src_len, sub, blocks] + list(starts) + list(keys)
    for table in (res, side, marks):
        for row in table:
            words += row
    out = subprocess.run([exe], input=" ".join(str(w) for w in words), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    status, numbers, copies, segs = out.stdout.strip("\n").split("\n")
    produced, end_bit, final, subparts = (int(x) for x in numbers.split())
    c = [int(x) for x in copies.split()[1:]]
    return (status, produced, end_bit, final, subparts, [tuple(c[i:i + 3]) for i in range(0, len(c), 3)],
            [int(x) for x in segs.split()[1:]])


def test_clean_chain_of_four_parts(driver):
    # each part ends on the next start; the last one ends the BFINAL block at bit 7990 of 8000
    res = [part(50000, 1000, link=1), part(60000, 2000, link=2, reach=32768), part(100, 3000, link=3), part(20000, 7990, ended=1)]
    got = walk(driver, [0, 1000, 2000, 3000], res)
    # segments: [0] closes at 50000 >= 40960, [1] at 60000, parts 2 + 3 are 20100 < 32768 symbols and join the second
    assert got == ("ok", 130100, 7990, 1, 0, [(0, 0, 50000), (1, 50000, 60000), (2, 110000, 100), (3, 110100, 20000)], [0, 1, 4])


def test_a_candidate_never_landed_on_is_skipped(driver):
    # start 1 was noise: part 0 ran across it and ended on start 2; what part 1 reports (a data error) is never looked at
    res = [part(50000, 2000, link=2), part(7, 1100, msg=LITLEN_CODE), part(41000, 3000, link=3), part(40000, 7000, ended=1),
           part(9, 7500, msg=LITLEN_CODE)]
    got = walk(driver, [0, 1000, 2000, 3000, 7100], res)
    assert got == ("ok", 131000, 7000, 1, 0, [(0, 0, 50000), (2, 50000, 41000), (3, 91000, 40000)], [0, 1, 2, 3])


def test_a_message_or_a_missing_end_on_the_chain_fails_at_that_part(driver):
    res = [part(50000, 1000, link=1), part(10, 1500, msg=LITLEN_CODE, link=2), part(5, 3000, ended=1)]
    assert walk(driver, [0, 1000, 2000], res)[0] == "fail 1 a part's message, or no end"
    res = [part(50000, 1000, link=1), part(10, 1500), part(5, 3000, ended=1)]        # not the end and no start landed on
    assert walk(driver, [0, 1000, 2000], res)[0] == "fail 1 a part's message, or no end"


@pytest.mark.parametrize("link", [1, 0, 4])       # itself, backwards, behind the stream's last part
def test_a_link_that_does_not_point_forward_inside_the_stream_fails(driver, link):
    res = [part(50000, 1000, link=1), part(100, 2000, link=link), part(100, 3000, link=3), part(100, 4000, ended=1)]
    got = walk(driver, [0, 1000, 2000, 3000], res)
    assert got[0] == "fail -1 bad chain link"
    assert got[5] == [(0, 0, 50000), (1, 50000, 100)]          # (it stopped there: no second visit)


def test_links_of_a_stream_inside_a_batch_table(driver):
    # the stream's parts are rows 3 .. 6 of a launch of 8: links are rows of the table; rows 2 and 7 belong to other streams
    other = part(1, 1, ended=1)
    mine = [part(50000, 1000, link=4), part(45000, 2000, link=5), part(100, 3000, link=6), part(100, 4000, ended=1)]
    res = [other] * 3 + mine + [other]
    got = walk(driver, [0, 1000, 2000, 3000], res, pbase=3)
    assert got == ("ok", 95200, 4000, 1, 0, [(3, 0, 50000), (4, 50000, 45000), (5, 95000, 100), (6, 95100, 100)], [0, 1, 4])
    for bad in (2, 7):
        res[4] = part(45000, 2000, link=bad)
        assert walk(driver, [0, 1000, 2000, 3000], res, pbase=3)[0] == "fail -1 bad chain link"


def test_a_distance_in_front_of_the_stream_fails(driver):
    # part 0 may reach window_len bytes back, part 1 those and part 0's 1000
    ok = [part(1000, 1000, link=1, reach=100), part(500, 2000, ended=1, reach=1100)]
    assert walk(driver, [0, 1000], ok, window_len=100)[:3] == ("ok", 1500, 2000)
    assert walk(driver, [0, 1000], ok, window_len=99)[0] == "fail -1 a distance reaches in front of the stream"
    far = [part(1000, 1000, link=1, reach=100), part(500, 2000, ended=1, reach=1101)]
    got = walk(driver, [0, 1000], far, window_len=100)
    assert got[0] == "fail -1 a distance reaches in front of the stream" and got[5] == [(0, 0, 1000)]


def test_a_fixed_code_sub_part_inside_the_final_block_ends_the_stream(driver):
    starts, keys = [0, 1000, 2000, 3000], [0, 1, 1, 0]
    # part 0 read a BFINAL header and handed off inside that block to part 1, whose first block -- the rest of it -- ended at
    # bit 1900 after 700 symbols; what part 1 decoded behind that (its result words) is not part of the stream
    res = [part(5000, 1000, link=1), part(9999, 3000, link=3), part(1, 2500, msg=LITLEN_CODE), part(1, 7000, ended=1)]
    side = [[NONE, 0, 0, 0, 1, 1, 0, 0], [700, 1900, 0, 30, 0, 0, 0, 0], NO_SIDE, NO_SIDE]
    got = walk(driver, starts, res, keys=keys, side=side, sub=1)
    assert got == ("ok", 5700, 1900, 1, 1, [(0, 0, 5000), (1, 5000, 700)], [0, 2])
    # its reach is checked like any part's, and its end has to lie inside the input (1000 bytes)
    side[1] = [700, 1900, 0, 5001, 0, 0, 0, 0]
    assert walk(driver, starts, res, keys=keys, side=side, sub=1)[0] == "fail -1 a distance reaches in front of the stream"
    side[1] = [700, 8001, 0, 30, 0, 0, 0, 0]
    assert walk(driver, starts, res, keys=keys, side=side, sub=1)[0] == "fail -1 the final block runs past the input"
    # the block part 0 handed off in was NOT final: part 1 is an ordinary link of the chain, and counts as a sub-part
    side[0], side[1] = [NONE, 0, 0, 0, 1, 0, 0, 0], [700, 1900, 0, 30, 0, 0, 0, 0]
    got = walk(driver, starts, res, keys=keys, side=side, sub=1)
    assert got == ("ok", 15000, 7000, 1, 1, [(0, 0, 5000), (1, 5000, 9999), (3, 14999, 1)], [0, 3])


def test_the_final_flag_is_carried_across_a_sub_part_still_in_its_first_block(driver):
    # part 1 began inside the BFINAL block and handed off to part 2 before that block ended (BFINAL word 2 = "unknown to
    # me"): part 2 still knows the block is final, and ends the stream at its first block's end
    starts, keys = [0, 1000, 2000], [0, 1, 1]
    res = [part(5000, 1000, link=1), part(800, 2000, link=2), part(4000, 6000, ended=1)]
    side = [[NONE, 0, 0, 0, 1, 1, 0, 0], [NONE, 0, 0, 0, 1, 2, 0, 0], [300, 2500, 0, 0, 0, 0, 0, 0]]
    got = walk(driver, starts, res, keys=keys, side=side, sub=1)
    assert got == ("ok", 6100, 2500, 1, 2, [(0, 0, 5000), (1, 5000, 800), (2, 5800, 300)], [0, 3])
    # a part that ended on a block boundary (no hand-off) clears it: part 2's own result counts
    side[1] = [NONE, 0, 0, 0, 0, 0, 0, 0]
    got = walk(driver, starts, res, keys=keys, side=side, sub=1)
    assert got == ("ok", 9800, 6000, 1, 1, [(0, 0, 5000), (1, 5000, 800), (2, 5800, 4000)], [0, 3])


def test_blocks_mode_keeps_the_complete_blocks_of_the_part_that_ran_out_of_input(driver):
    res = [part(50000, 1000, link=1), part(900, 8000, msg=STARVED)]
    marks = [[0, 0, 0, 0], [300, 1500, 0, 10]]
    got = walk(driver, [0, 1000], res, marks=marks, blocks=1)
    assert got == ("ok", 50300, 1500, 0, 0, [(0, 0, 50000), (1, 50000, 300)], [0, 2])
    assert walk(driver, [0, 1000], res, marks=marks)[0] == "fail 1 a part's message, or no end"       # stream mode: truncated


@pytest.mark.parametrize("sizes, segs", [
    ([100], [0, 1]),                              # a single short segment stands
    ([50000, 32767], [0, 2]),                     # a tail below 32768 joins the segment in front
    ([50000, 32768], [0, 1, 2]),                  # a segment's worth of tail stands
    ([20000, 20000, 960, 40959, 1, 70000], [0, 3, 5, 6]),      # closed at exactly 40960; 40959 + 1 likewise
])
def test_segments(driver, sizes, segs):
    starts = [1000 * i for i in range(len(sizes))]
    res = [part(n, 1000 * (i + 1), link=i + 1) for i, n in enumerate(sizes[:-1])] + [part(sizes[-1], 1000 * len(sizes), ended=1)]
    got = walk(driver, starts, res)
    assert got[0] == "ok" and got[1] == sum(sizes) and got[6] == segs


def rule(exe, name, words):
    """-> {line name: [numbers]} of the driver's `name` rule (a line without a name: "")"""
    out = subprocess.run([exe, name], input=" ".join(str(w) for w in words), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = {}
    for ln in out.stdout.strip("\n").split("\n"):
        head, _, rest = ln.partition(":") if ":" in ln else ("", "", ln)
        got[head] = [int(x) for x in rest.split()]
    return got


@pytest.mark.parametrize("np_, sub, blocks, want", [
    # jobs, starts, keys, res, extra, up_bytes, res_words, mirror; 40 np, 8 np (16 np), 32 np (+ 16 np, + 32 np), each up to 256
    (1, 0, 0, (0, 256, 264, 512, 544, 264, 8, 768)),
    (1, 1, 0, (0, 256, 264, 512, 544, 272, 16, 768)),
    (1, 0, 1, (0, 256, 264, 512, 544, 264, 12, 768)),
    (5, 0, 0, (0, 256, 296, 512, 672, 296, 8, 768)),
    (5, 1, 0, (0, 256, 296, 512, 672, 336, 16, 1024)),            # results | side words: 320 bytes -> 512
    (5, 0, 1, (0, 256, 296, 512, 672, 296, 12, 768)),             # results | marks: 240 bytes
])
def test_part_table_layout(driver, np_, sub, blocks, want):
    slot_symbols = 123456
    jobs, starts, keys, res, extra, slots, up, res_words, mirror, device = rule(driver, "layout", [np_, sub, blocks, slot_symbols])[""]
    assert (jobs, starts, keys, res, extra, up, res_words, mirror) == want
    # 256-aligned, in order and not overlapping: each table ends before the next begins
    assert all(o % 256 == 0 for o in (jobs, starts, res, slots))
    assert jobs + 40 * np_ <= starts and starts + (16 if sub else 8) * np_ <= res and res + 4 * res_words * np_ <= slots
    assert keys == starts + 8 * np_                               # the keys follow the starts ...
    assert up == starts + (16 if sub else 8) * np_                # ... and go up with them and the jobs
    assert extra == res + 32 * np_                                # marks or side words follow the 8 result words per part
    assert res_words == 8 + (4 if blocks else 0) + (8 if sub else 0)
    assert slots == mirror and device == mirror + 2 * slot_symbols


def retry_cap(part_bytes):
    return (part_bytes * 1032 + (640 << 10) + 7) & ~7


def test_retry_plan(driver):
    # two streams of 3 and 2 parts; parts 1 and 4 were full
    spans, part_bytes = [0, 3, 3, 2], [100, 200, 300, 400, 500]
    msgs = [0, OUT_FULL, 0, LITLEN_CODE, OUT_FULL]
    assert (retry_cap(200), retry_cap(500)) == (861760, 1171360)
    got = rule(driver, "retry", [24 << 30, 2] + spans + [5] + part_bytes + msgs)
    assert got == {"again": [1, 4], "off": [0, 861760], "cap": [861760, 1171360], "total": [2033120], "over": []}
    # the second stream wants 2 x 1171360 bytes: one byte less is over its limit, and the first stream's part is still planned
    got = rule(driver, "retry", [2 * 1171360 - 1, 2] + spans + [5] + part_bytes + msgs)
    assert got == {"again": [1], "off": [0], "cap": [861760], "total": [861760], "over": [1]}
    got = rule(driver, "retry", [2 * 1171360, 2] + spans + [5] + part_bytes + msgs)
    assert got["again"] == [1, 4] and got["over"] == []
    # no part full: nothing to run again
    got = rule(driver, "retry", [24 << 30, 2] + spans + [5] + part_bytes + [0, 0, STARVED, 0, 0])
    assert got == {"again": [], "off": [], "cap": [], "total": [0], "over": []}


def test_the_first_full_part_on_the_chain(driver):
    """a piece over its retry cap runs the full parts ON its chain again, one at a time: parts that no chain reaches (noise
    candidates -- a stored block's payload may hold thousands of headers that promise 65535 bytes each) ask for nothing"""
    none = 0xffffffff

    def ask(i0, i1, rows):
        out = subprocess.run([driver, "chainfull"], input=" ".join(str(x) for x in [i0, i1, len(rows)] + [v for r in rows for v in r]),
                             capture_output=True, text=True, check=True).stdout.strip()
        return out if out in ("end", "broken") else int(out)
    ok, full, err = (lambda link: (0, 0, link)), (OUT_FULL, 0, none), (LITLEN_CODE, 0, none)
    # the chain 0 -> 3 -> 5 -> 7 (BFINAL) among full decoys: it meets none of them
    rows = [ok(3), full, full, ok(5), full, ok(7), full, (0, 1, none)]
    assert ask(0, 8, rows) == "end"
    assert ask(0, 8, rows[:5] + [(STARVED, 0, none)] + rows[6:]) == "end"          # a piece: the chain ends where the input does
    # part 5 is full: found; run again (a message of its own now) the walk goes on to part 7
    assert ask(0, 8, rows[:5] + [full] + rows[6:]) == 5
    assert ask(0, 8, [full] + rows[1:]) == 0
    assert ask(0, 8, rows[:7] + [full]) == 7
    # a chain that breaks: a message, a link that goes back or stays, a link out of the stream, no link and no end
    assert ask(0, 8, rows[:3] + [err] + rows[4:]) == "broken"
    for link in (2, 3, 8, none):
        assert ask(0, 8, rows[:3] + [ok(link)] + rows[4:]) == "broken", link
    # rows [2, 6) of a launch's tables: links are rows of the tables
    assert ask(2, 6, [full, full, ok(4), full, ok(5), (0, 1, none), full]) == "end"
    assert ask(2, 6, [full, full, ok(4), full, ok(6), (0, 1, none), full]) == "broken"
    assert ask(2, 6, [full, full, ok(3), full, ok(5), (0, 1, none), full]) == 3


KiB, MiB = 1 << 10, 1 << 20
FIND_LENS = [128 * KiB, 128 * KiB + 1, MiB + 4095, 256 * MiB, (1 << 31) - 1]
TAG_SHIFT, STORED, BEHIND_MARKER = 40, 1 << 62, 1 << 63       # kFindTagShift; a survivor's marks


def finder(exe, lens, survivors=()):
    """-> ((item_bytes, share), cap1, cap2, first, [(stream, lo, hi)], [patterns_first per stream], [sorted list per stream])"""
    words = [len(lens)] + list(lens) + [len(survivors)] + list(survivors)
    out = subprocess.run([exe, "finder"], input=" ".join(str(w) for w in words), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = [[int(x) for x in ln.split()[1:]] for ln in out.stdout.strip("\n").split("\n")]
    (item_bytes, cap1, cap2, first, nitems, share), items, pfirst, lists = rows[0], rows[1], rows[2], rows[3:]
    assert len(items) == 3 * nitems and len(pfirst) == len(lens) and len(lists) == len(lens)
    return (item_bytes, share), cap1, cap2, first, [tuple(items[i:i + 3]) for i in range(0, len(items), 3)], pfirst, lists


@pytest.mark.parametrize("lens", [[n] for n in FIND_LENS] + [FIND_LENS], ids=lambda v: "+".join(str(n) for n in v))
def test_finder_items_and_caps(driver, lens):
    """one finder pass: a stream's work items tile it in order, equal ones, as few as stay within a 4096th of the pass's bytes
    (4 .. 64 KiB) -- so one stream of up to 256 MiB is cut into 4096, as many as the chip takes in two rounds; room for a survivor per 64 (F1) and per 512 bytes (F2, the
    patterns) of the pass and 4096 per stream; one stream is a table of one, with the bounds decoy_cases.py restates"""
    import decoy_cases as dcy
    ns, total = len(lens), sum(lens)
    (item_bytes, share), cap1, cap2, first, items, pfirst, _ = finder(driver, lens)
    assert item_bytes == max(4096, min(65536, (total // 4096 + 4095) & ~4095))
    assert item_bytes % 4096 == 0 and 4096 <= item_bytes <= 65536
    assert share == max(4096, min(item_bytes, -(-total // 4096)))
    assert [k for k, _, _ in items] == sorted(k for k, _, _ in items)        # the streams in the table's order
    assert len(items) == sum(-(-n // share) for n in lens)                   # as many as the plan counts, and no others
    for k, n in enumerate(lens):
        own = [(lo, hi) for s, lo, hi in items if s == k]
        assert own[0][0] == 0 and own[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(own, own[1:]))               # no gap, no overlap
        assert all(0 < hi - lo <= share <= item_bytes for lo, hi in own)
        assert len(own) == -(-n // share)
        assert all(hi - lo == -(-n // len(own)) for lo, hi in own[:-1])      # equal shares; the last one has what is left
    assert (cap1, cap2) == (total // 64 + 4096 * ns, total // 512 + 4096 * ns) and cap1 < 1 << 32
    assert first == min(cap2, 16384 + 64 * ns)
    assert pfirst == [dcy.patterns_first(n) for n in lens]
    if ns == 1:
        assert len(items) == (4096 if (16 << 20) <= total <= (256 << 20) else -(-total // share))
        assert cap2 == dcy.cap2(lens[0]) and cap1 == min(lens[0] // 64 + 4096, 64 << 20)
        assert first >= pfirst[0]                         # whether the patterns cut the stream is known without a second copy


def test_finder_survivors_go_to_their_stream_sorted(driver):
    def tagged(k, bit, marks=0):
        return (k << TAG_SHIFT) | bit | marks
    got = [tagged(0, 90, STORED | BEHIND_MARKER), tagged(1, 800), tagged(0, 50, BEHIND_MARKER), tagged(3, 5),
           tagged(2, 7), tagged(0, 80), tagged(0x3fffff, 1), tagged(0, 70, STORED | BEHIND_MARKER), tagged(1, 16, BEHIND_MARKER)]
    lists = finder(driver, [128 * KiB] * 3, got)[6]
    # by its tag, which comes off with bit 63; tags 3 and 0x3fffff name no stream of a table of three; bit 62 stays and does
    # not count in the order (by_bit: a sort by value would put 80 in front of 70 | STORED)
    assert lists == [[50, 70 | STORED, 80, 90 | STORED], [16, 800], [7]]
    assert finder(driver, [128 * KiB], [tagged(0, 9), tagged(1, 3), tagged(0, 4, BEHIND_MARKER)])[6] == [[4, 9]]


def test_symbol_tables_of_one_stream(driver):
    # three copies: 30000 + 20000 close a segment (50000 >= 40960), the third (50000 >= 32768) is one of its own
    got = rule(driver, "segs", [1, 100000, 7000000, 3, 0, 30000, 30000, 20000, 50000, 50000])
    assert got["v"] == [32768]
    assert got["copies"] == [0, 32768, 32768, 30000, 0,
                             1, 62768, 32768, 20000, 0,
                             2, 82768, 82768, 50000, 2]
    assert got["segs"] == [32768 + 0, 32768 + 50000, 32768 + 100000]          # the last: the closing triple
    assert got["seg_dst"] == [7000000, 7050000]
    assert got["seg_end"] == [82768, 32768 + 100000]
    assert got["v_end"] == [132768]


def test_symbol_tables_of_streams_one_behind_the_other(driver):
    first = [100000, 7000000, 3, 0, 30000, 30000, 20000, 50000, 50000]
    nothing = [0, 8000000, 1, 0, 0]                               # produced nothing: no place in the array
    second = [40000, 9000000, 2, 0, 15000, 15000, 25000]
    got = rule(driver, "segs", [3] + first + nothing + second)
    v2 = 132768 + 32768                                           # behind the first stream's end and its own gap
    assert got["v"] == [32768, 0, v2]
    # the second stream's copies are numbers 4 and 5 of the input (slot) and 3 and 4 of the table: its one segment begins at 3
    assert got["copies"][15:] == [4, v2, v2, 15000, 3, 5, v2 + 15000, v2, 25000, 3]
    assert got["copies"][:15] == [0, 32768, 32768, 30000, 0, 1, 62768, 32768, 20000, 0, 2, 82768, 82768, 50000, 2]
    assert got["segs"] == [32768, 82768, v2, v2 + 40000]
    assert got["seg_dst"] == [7000000, 7050000, 9000000]           # its own destination
    assert got["seg_end"] == [82768, 132768, v2 + 40000]
    assert got["v_end"] == [v2 + 40000]


# ---- the pieces loop's rules ------------------------------------------------------------------------------------------------
PIECE_MIN = 4 * MiB                               # kPieceMin
IN_DST, WINDOW, SPLICED = 0, 1, 2                 # PieceHistory::Where


def pieces(exe, op, words):
    """-> the numbers of every output line of the driver's `pieces` operation `op`, in order"""
    out = subprocess.run([exe, "pieces"], input=" ".join(str(w) for w in [op] + list(words)), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return [[int(x) for x in ln.split()[1:]] for ln in out.stdout.strip("\n").split("\n")]


def state(bit=0, key=0, fin=-1, produced=0, abit=0, aout=0, p=PIECE_MIN):
    return [bit, key, fin, produced, abit, aout, p]


def next_piece(exe, st, src_len, piece_bytes=PIECE_MIN):
    """-> dict of piece_next's answer"""
    (any_, end, base, start_bit, scan_lo, key0), (fin0,), (last, q) = pieces(exe, "next", st + [src_len, piece_bytes])
    return dict(any=any_, end=end, base=base, start_bit=start_bit, scan_lo=scan_lo, key0=key0, fin0=fin0, last=last, q=q)


@pytest.mark.parametrize("bit, p, src_len, end, last", [
    (0, PIECE_MIN, 300000, 300000, 1),                                    # a stream shorter than one piece
    (0, PIECE_MIN, PIECE_MIN, PIECE_MIN, 1),                              # exactly one piece
    (0, PIECE_MIN, PIECE_MIN + MiB, PIECE_MIN, 0),                        # a tail of exactly a quarter piece: not shortened
    (0, PIECE_MIN, PIECE_MIN + MiB - 1, PIECE_MIN - 1, 0),                # one byte less: a quarter piece is left behind
    (8 * 1000 + 3, PIECE_MIN, 1000 + PIECE_MIN + MiB - 1, 1000 + PIECE_MIN - 1, 0),       # the same from byte 1000
    (0, PIECE_MIN, PIECE_MIN + 1, PIECE_MIN + 1 - MiB, 0),                # a tail of one byte
    (8 * PIECE_MIN, PIECE_MIN, PIECE_MIN + 5, PIECE_MIN + 5, 1),          # the last piece
    (0, 2 * MiB, 2 * MiB + MiB // 2 - 1, 2 * MiB - 1, 0),                 # a halved piece: a quarter of ITS size
])
def test_where_a_piece_ends(driver, bit, p, src_len, end, last):
    got = next_piece(driver, state(bit=bit, p=p), src_len, piece_bytes=2 * PIECE_MIN)
    assert (got["any"], got["end"], got["last"]) == (1, end, last)
    assert got["end"] > bit >> 3                                          # never in front of its start
    assert got["q"] == 2 * PIECE_MIN and got["fin0"] == -1                # the caps go by the call's piece size, not by p


def test_no_piece_behind_the_last_byte(driver):
    assert next_piece(driver, state(bit=8 * 5000), 5000)["any"] == 0
    assert next_piece(driver, state(bit=8 * 5000 + 7), 5001)["any"] == 1


@pytest.mark.parametrize("bit, key, base, scan_lo, start_bit, key0", [
    (8003, 0, 768, 232, 8003 - 6144, 0),                                  # byte 1000 is no multiple of 256: base 768
    (8003, 1, 768, 232, 1859, 1),                                         # keys 0 and 1 are no positions: as they are
    # H = bit 1 of byte 99000, 1000 bytes in front of the piece's byte 100000: base = 99000 & ~255 = 98816, 8 base = 790528
    (800005, 792001 + 2, 98816, 1184, 800005 - 790528, 792003 - 790528),
    # H = bit 7 of byte 99990, 10 bytes in front: base = 99840, 8 base = 798720
    (800005, 799927 + 2, 99840, 160, 800005 - 798720, 799929 - 798720),
    # H in the piece's first byte itself (bit 1 of byte 100000; the start is bit 5)
    (800005, 800001 + 2, 99840, 160, 1285, 800003 - 798720),
])
def test_where_the_pass_buffer_begins_and_what_is_rebased(driver, bit, key, base, scan_lo, start_bit, key0):
    st = state(bit=bit, key=key, fin=1, produced=5000, abit=4000, aout=700)
    got = next_piece(driver, st, 10 * MiB)
    assert (got["base"], got["scan_lo"], got["start_bit"], got["key0"], got["fin0"]) == (base, scan_lo, start_bit, key0, 1)
    assert got["scan_lo"] + got["base"] == bit >> 3 and got["base"] % 256 == 0
    if key >= 2:
        assert (key0 - 2) >> 3 == ((key - 2) >> 3) - base                 # the header lies in the buffer, at its own byte
    # a pass that stops at its own first start with its own key hands back the bit and the key that went in
    step, after = pieces(driver, "pass", st + [10 * MiB, PIECE_MIN, 1, start_bit, key0, 1, 0, 0])
    assert step == [0, 0, 1 if key == 0 else 0]
    assert after[:3] == [bit, key, 1]


def test_the_state_behind_a_pass(driver):
    # the piece begins at bit 5 of byte 100000 inside the dynamic block at bit 792001: base 98816 (above); p had been halved
    st = state(bit=800005, key=792003, fin=1, produced=5000, abit=700000, aout=4000, p=2 * MiB)
    run = lambda *said: pieces(driver, "pass", st + [10 * MiB, PIECE_MIN] + list(said))
    # stopped at a block start, bit 20000 of the buffer, behind 7000 bytes: the anchor moves there
    assert run(1, 20000, 0, -1, 7000, 0) == [[0, 0, 1], [810528, 0, -1, 12000, 810528, 12000, PIECE_MIN]]
    # stopped inside a fixed-code block whose BFINAL the chain knows: the anchor stays, fin is carried
    assert run(1, 20000, 1, 1, 7000, 0) == [[0, 0, 0], [810528, 1, 1, 12000, 700000, 4000, PIECE_MIN]]
    # stopped inside the dynamic block at bit 15000 of the buffer: its key goes back by 8 base
    assert run(1, 20000, 15002, 0, 7000, 0) == [[0, 0, 0], [810528, 15002 + 790528, 0, 12000, 700000, 4000, PIECE_MIN]]
    # not stopped: the stream ended 123456 bytes into the buffer
    step, after = run(0, 0, 0, -1, 7000, 123456)
    assert step == [1, 98816 + 123456, 0] and after[3] == 12000


def test_halving_stops_at_the_least_piece(driver):
    assert pieces(driver, "halve", [2 * PIECE_MIN]) == [[1, PIECE_MIN]]
    assert pieces(driver, "halve", [2 * PIECE_MIN - 1]) == [[0, 2 * PIECE_MIN - 1]]
    assert pieces(driver, "halve", [PIECE_MIN]) == [[0, PIECE_MIN]]
    assert pieces(driver, "halve", [64 * MiB]) == [[1, 32 * MiB]]


@pytest.mark.parametrize("pos, window_len, want", [
    # len, where, dst_off, window_off, from_window, from_dst
    (0, 0, [0, IN_DST, 0, 0, 0, 0]),                                       # nothing in front: no history
    (0, 1000, [1000, WINDOW, 0, 0, 0, 0]),                                # the caller's window as it stands
    (0, 32768, [32768, WINDOW, 0, 0, 0, 0]),
    (100, 0, [100, IN_DST, 0, 0, 0, 0]),                                  # no window: what was delivered
    (100, 200, [300, SPLICED, 0, 0, 200, 100]),                           # pos + window_len < 32768: all of both
    (20000, 20000, [32768, SPLICED, 0, 7232, 12768, 20000]),              # pos < 32768 <= pos + window_len: the window's end
    (30000, 32768, [32768, SPLICED, 0, 30000, 2768, 30000]),
    (32767, 5, [32768, SPLICED, 0, 4, 1, 32767]),
    (32768, 32768, [32768, IN_DST, 0, 0, 0, 0]),                          # pos >= 32768: the output has it all
    (100000, 0, [32768, IN_DST, 67232, 0, 0, 0]),
])
def test_the_history_in_front_of_an_output_position(driver, pos, window_len, want):
    assert pieces(driver, "history", [pos, window_len]) == [want]


def test_the_sequential_decoders_input(driver):
    # the anchor is bit 5 of byte 10 MiB, the piece the device could not do begins 40 MiB behind it: that piece whole
    far = state(bit=8 * 50 * MiB + 3, abit=8 * 10 * MiB + 5, p=PIECE_MIN)
    got = pieces(driver, "seq", far + [100 * MiB, 3, 0, 5, 0, 5, 0, 5])
    assert got[0] == [10 * MiB, 5, 44 * MiB, 44 * MiB]
    # no block completed (status 0, the end bit still 5): twice as much, until all 90 MiB behind the anchor were given --
    # then the stream form says how the stream ends
    assert got[1:] == [[1, 88 * MiB, 88 * MiB, 1], [1, 176 * MiB, 90 * MiB, 1], [0, 176 * MiB, 90 * MiB, 1]]
    # the piece begins at the anchor: two pieces
    near = state(bit=8 * 10 * MiB + 5, abit=8 * 10 * MiB + 5, p=PIECE_MIN)
    assert pieces(driver, "seq", near + [100 * MiB, 0])[0] == [10 * MiB, 5, 8 * MiB, 8 * MiB]
    assert pieces(driver, "seq", near + [12 * MiB, 0])[0] == [10 * MiB, 5, 8 * MiB, 2 * MiB]
    # a block completed: no more input is asked for, whatever is left
    assert pieces(driver, "seq", near + [100 * MiB, 1, 0, 900])[1] == [0, 8 * MiB, 8 * MiB, 0]


@pytest.mark.parametrize("status, moved, stream_form", [
    (1, True, 0), (1, False, 0),                  # the stream ended in the blocks form
    (0, True, 0),                                 # complete blocks: delivered, and the device goes on
    (0, False, 1),                                # the input ends inside the first block
    (-3, True, 1), (-3, False, 1),                # a data error: the stream form's message and counts
    (-4, True, 0), (-4, False, 0),                # out of memory: no second attempt
    (-5, False, 1), (2, True, 1),                 # anything else the decoder might say
])
def test_which_form_of_the_sequential_decoder_answers(driver, status, moved, stream_form):
    # all of the input was given (4000 bytes behind byte 1000), so nothing is doubled
    st = state(bit=8 * 1000 + 5, abit=8 * 1000 + 5)
    got = pieces(driver, "seq", st + [5000, 1, status, 77 if moved else 5])
    assert got == [[1000, 5, 8 * MiB, 4000], [0, 8 * MiB, 4000, stream_form]]
    assert stream_form == int(status != 1 and not (status == 0 and moved) and status != -4)


def test_the_state_behind_the_sequential_decoders_blocks(driver):
    st = state(bit=8 * 50 * MiB + 3, key=792003, fin=1, produced=9000, abit=8 * 10 * MiB + 5, aout=4000, p=2 * MiB)
    # complete blocks up to bit 1000005 from byte 10 MiB, 14000 bytes delivered with them: a block start, the new anchor
    at = 8 * 10 * MiB + 1000005
    assert pieces(driver, "blocks", st + [1000005, 14000, PIECE_MIN]) == [[at, 0, -1, 14000, at, 14000, PIECE_MIN]]
