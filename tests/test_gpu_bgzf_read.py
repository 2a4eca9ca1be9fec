"""BGZF random access on the device, through the C ABI: zng_rocm_bgzf_index_dev (the members table without decoding),
zng_rocm_bgzf_read_dev (many plaintext ranges in one set of launches) and the virtual offsets.
Oracle: CPython's loop of zlib.decompressobj(31) over unused_data (gzip_files.oracle_table) for the rows and the plaintext, and
Python slicing for the ranges.  The file sits at an odd device address; every destination sits at a chosen address modulo 16
inside one arena of 0xAB, and `Arena.check` asserts that no byte outside the destinations changed."""
import ctypes as C
import gzip
import importlib
import os
import zlib

import numpy as np
import pytest

from gzip_files import BGZF_BLOCK, BGZF_EOF, bgzf_block, bgzf_file, oracle_table
from wrapped_members import place

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, DATA_ERROR, BUF_ERROR = -3, -3, -5
ROW_MSG = "index row does not match the file"
KiB = 1 << 10


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.deflate"), importlib.import_module("zlib-ng_amd.inflate"), zr


@pytest.fixture(scope="module")
def lcet():
    with open(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "data_lcet10.txt"), "rb") as f:
        return f.read()[:200000]


class File:
    """a file in device memory at an address `odd` modulo 16, with the oracle's rows and plaintext when it is well-formed"""

    def __init__(self, mods, data, odd=3, oracle=True):
        self.data = bytes(data)
        self.src = place(mods[0], self.data, odd)
        if oracle:
            self.rows, self.plain, self.end = oracle_table(self.data)


@pytest.fixture(scope="module")
def tiny(mods, lcet):
    """about 21 members of 997 bytes and the end-of-file block"""
    return File(mods, bgzf_file(lcet[:20000], block=997))


@pytest.fixture(scope="module")
def holed(mods, lcet):
    """the same with an empty member in the middle: members 0..9, an empty one, members 11..21, the end-of-file block"""
    blocks = [bgzf_block(lcet[at:min(at + 997, 20000)]) for at in range(0, 20000, 997)]
    return File(mods, b"".join(blocks[:10]) + bgzf_block(b"") + b"".join(blocks[10:]) + BGZF_EOF, odd=5)


@pytest.fixture(scope="module")
def big3(mods, lcet):
    """three members of 65280 bytes"""
    return File(mods, bgzf_file(lcet[:3 * BGZF_BLOCK]), odd=7)


def index(mods, f, **kw):
    torch, _, inf, zr = mods
    out = inf.bgzf_index_dev(f.src, **kw)
    torch.cuda.synchronize()
    return out + (zr.rocm.lib().zng_rocm_last_error().decode(),)


def gunzip(mods, f):
    torch, _, inf, _ = mods
    dst = torch.zeros(max(len(getattr(f, "plain", b"")), 1 << 20), dtype=torch.uint8, device="cuda")
    out = inf.gunzip_members_dev(f.src, dst)
    torch.cuda.synchronize()
    return out


# ---- the index --------------------------------------------------------------------------------------------------------------
def check_index(mods, f):
    st, rows, nmembers, plain_len, in_used, _ = index(mods, f)
    assert (st, nmembers, plain_len, in_used) == (0, len(f.rows), len(f.plain), f.end)
    assert rows == f.rows
    gst, gout, gused, grows, gn, _ = gunzip(mods, f)
    assert (gst, gout, gused, gn) == (1, plain_len, in_used, nmembers) and grows == rows


def test_index_tiny_members(mods, tiny):
    assert len(tiny.rows) == 22 and tiny.rows[-1][1:4] == (28, 20000, 0)
    check_index(mods, tiny)


def test_index_empty_member_in_the_middle(mods, holed):
    assert len(holed.rows) == 23 and holed.rows[10][3] == 0
    check_index(mods, holed)


def test_index_full_members(mods, big3):
    assert [r[3] for r in big3.rows] == [BGZF_BLOCK] * 3 + [0]
    check_index(mods, big3)


def test_index_extra_subfields_around_bc(mods, lcet):
    data = bgzf_block(lcet[:5000], extra_front=b"XY\x03\x00abc") + bgzf_block(lcet[5000:9000], extra_behind=b"ZZ\x00\x00") + \
        bgzf_block(lcet[9000:9500], extra_front=b"BC\x03\x00123", extra_behind=b"QQ\x01\x00q") + BGZF_EOF
    f = File(mods, data)
    assert [r[5] for r in f.rows] == [1, 1, 1, 1] and f.plain == lcet[:9500]
    check_index(mods, f)


def test_index_members_cap(mods, tiny):
    for cap in (0, 1, 5, 21, 22, 40):
        st, rows, nmembers, plain_len, in_used, _ = index(mods, tiny, members_cap=cap)
        assert (st, nmembers, plain_len, in_used) == (0, 22, 20000, len(tiny.data)) and rows == tiny.rows[:cap], cap
    torch, _, inf, zr = mods                                                # rows behind members_cap stay as they are
    size = C.sizeof(inf.GzipMember)
    table = np.full(7 * size, 0xCD, dtype=np.uint8)
    n, p, u = C.c_size_t(0), C.c_uint64(0), C.c_size_t(0)
    st = zr.rocm.lib().zng_rocm_bgzf_index_dev(tiny.src.data_ptr(), len(tiny.data), C.c_void_p(table.ctypes.data), 5, C.byref(n), C.byref(p),
                                               C.byref(u), None)
    assert (st, n.value) == (0, 22) and bytes(table[5 * size:]) == b"\xcd" * (2 * size)


def test_index_candidate_inside_a_member(mods, lcet):
    # a stored block shows its plaintext as it is: whole BGZF headers, and a member that would end behind the file
    inner = BGZF_EOF * 3 + bgzf_block(lcet[:3000])[:18] + b"\x1f\x8b\x08\x04" + lcet[:500]
    data = bgzf_block(lcet[:700]) + bgzf_block(inner, level=0) + bgzf_block(lcet[700:900]) + BGZF_EOF
    f = File(mods, data)
    assert data.count(b"\x1f\x8b\x08\x04") >= 4 + 5 and len(f.rows) == 4
    check_index(mods, f)
    assert gunzip(mods, f)[5]["candidates"] >= 9


@pytest.mark.parametrize("tail", [b"", b"\x00", b"\x1f", b"ab", b"\x1f\x8c junk", bytes(100)])
def test_index_trailing_garbage(mods, tiny, tail):
    f = File(mods, tiny.data + tail, oracle=False)
    st, rows, nmembers, plain_len, in_used, _ = index(mods, f)
    assert (st, nmembers, plain_len, in_used) == (0, 22, 20000, len(tiny.data)) and rows == tiny.rows


def test_index_plain_gzip_member_behind_two_bgzf_members(mods, lcet):
    two = bgzf_block(lcet[:3000]) + bgzf_block(lcet[3000:4000])
    want, _, _ = oracle_table(two)
    for third in (gzip.compress(lcet[:1000]), b"\x1f\x8b\x09\x00" + bytes(40), b"\x1f\x8b\x09\x00"):
        f = File(mods, two + third, oracle=False)
        st, rows, nmembers, plain_len, in_used, err = index(mods, f)
        assert (st, nmembers, plain_len, in_used) == (DATA_ERROR, 2, 4000, len(two)) and rows == want, third[:4]
        assert "offset %d" % len(two) in err
    # at offset 0 nothing is in front: a plain gzip file is refused, with no members
    f = File(mods, gzip.compress(lcet[:1000]), oracle=False)
    assert index(mods, f)[:5] == (DATA_ERROR, [], 0, 0, 0)


def test_index_file_cut_inside_the_last_member(mods, tiny):
    last = tiny.rows[-2]
    for cut in (last[0] + last[1] - 1, last[0] + last[1] - 9, last[0] + 18, last[0] + 17, last[0] + 11, last[0] + 2):
        f = File(mods, tiny.data[:cut], oracle=False)
        st, rows, nmembers, plain_len, in_used, err = index(mods, f)
        assert (st, nmembers, plain_len, in_used) == (BUF_ERROR, 20, last[2], last[0]) and rows == tiny.rows[:20], cut
        assert "offset %d" % last[0] in err
    f = File(mods, tiny.data[:last[0] + 1], oracle=False)                   # one byte behind a member is garbage
    assert index(mods, f)[0:5] == (0, tiny.rows[:20], 20, last[2], last[0])
    f = File(mods, tiny.data[:10], oracle=False)
    assert index(mods, f)[0:5] == (BUF_ERROR, [], 0, 0, 0)


def test_index_does_not_decode(mods, tiny):
    off, used = tiny.rows[1][0], tiny.rows[1][1]
    bad = bytearray(tiny.data)
    bad[off + 18 + (used - 26) // 2] ^= 0x10                                # one payload byte of the second member
    f = File(mods, bad, oracle=False)
    st, rows, nmembers, plain_len, in_used, _ = index(mods, f)
    assert (st, nmembers, plain_len, in_used) == (0, 22, 20000, len(tiny.data)) and rows == tiny.rows
    assert gunzip(mods, f)[0] == DATA_ERROR


def test_index_empty_file_and_refusals(mods, tiny):
    torch, _, inf, zr = mods
    lib = zr.rocm.lib()
    assert inf.bgzf_index_dev(torch.zeros(0, dtype=torch.uint8, device="cuda")) == (0, [], 0, 0, 0)
    table = np.zeros(4 * C.sizeof(inf.GzipMember), dtype=np.uint8)
    for null in ("src", "members", "nmembers", "plain_len", "in_used"):
        n, p, u = C.c_size_t(77), C.c_uint64(77), C.c_size_t(77)
        st = lib.zng_rocm_bgzf_index_dev(None if null == "src" else tiny.src.data_ptr(), len(tiny.data),
                                         None if null == "members" else C.c_void_p(table.ctypes.data), 4,
                                         None if null == "nmembers" else C.byref(n), None if null == "plain_len" else C.byref(p),
                                         None if null == "in_used" else C.byref(u), None)
        assert st == EINVAL and not table.any(), null
        assert (n.value, p.value, u.value) == tuple(77 if null == k else 0 for k in ("nmembers", "plain_len", "in_used")), null


# ---- reading ----------------------------------------------------------------------------------------------------------------
class Arena:
    """one buffer of 0xAB with a destination per range: ranges = [(uoff, len)], odds = destination address modulo 16"""

    def __init__(self, torch, ranges, odds=None):
        self.torch = torch
        self.at, size = [], 64
        for k, (_, n) in enumerate(ranges):
            odd = (2 * k + 1) % 16 if odds is None else odds[k]
            size = (size + 15) // 16 * 16 + odd
            self.at.append(size)
            size += n + 33
        self.lens = [n for _, n in ranges]
        self.buf = torch.full((size + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.ptrs = [self.buf.data_ptr() + a for a in self.at]

    def check(self):
        """the destinations' bytes; everything else must still be 0xAB"""
        self.torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        mask = np.ones(host.size, dtype=bool)
        for a, n in zip(self.at, self.lens):
            mask[a:a + n] = False
        assert (host[mask] == 0xAB).all(), "a byte outside every destination was written"
        return [host[a:a + n].tobytes() for a, n in zip(self.at, self.lens)]


def read(mods, f, rows, ranges, odds=None, scratch=0):
    torch, _, inf, _ = mods
    arena = Arena(torch, ranges, odds)
    torch.cuda.synchronize()
    st, res, counters = inf.bgzf_read_dev(f.src, rows, [(u, n, p) for (u, n), p in zip(ranges, arena.ptrs)], scratch_bytes=scratch)
    return st, res, counters, arena.check()


def planned(rows, ranges):
    """(members through the engine, of those interior, distinct edges): an interior member per range it lies in, an edge once"""
    plain_len = rows[-1][2] + rows[-1][3]
    direct, edges = 0, set()
    for u, n in ranges:
        n = max(0, min(n, plain_len - u))
        for k, (_, _, dst_off, out_len, _, _) in enumerate(rows):
            if n and out_len and dst_off < u + n and dst_off + out_len > u:
                if dst_off >= u and dst_off + out_len <= u + n:
                    direct += 1
                else:
                    edges.add(k)
    return direct + len(edges), direct, len(edges)


def check_clean(f, ranges, st, res, got):
    assert st == 0
    for (u, n), (status, out_len, msg), data in zip(ranges, res, got):
        want = f.plain[u:u + n]
        assert (status, out_len, msg) == (1, len(want), None), (u, n, status, out_len, msg)
        assert data == want + b"\xab" * (n - len(want)), (u, n)


HOLED_RANGES = [(500, 0),                       # len 0
                (1000, 200),                    # inside member 1
                (997 * 3, 997),                 # exactly member 3
                (997 * 4 + 100, 997 * 3),       # edge 4, interiors 5 and 6, edge 7
                (997 * 9 + 5, 997 * 2),         # through the empty member: edge 9, interior, edge
                (19000, 1000),                  # to the end of the file: an edge, then the last member whole
                (20000, 10), (30000, 5),        # at and beyond the end
                (19990, 100),                   # clipped
                (1100, 50)]                     # shares edge member 1


def test_read_every_shape_in_one_call(mods, holed):
    st, res, counters, got = read(mods, holed, holed.rows, HOLED_RANGES)
    check_clean(holed, HOLED_RANGES, st, res, got)
    decoded, direct, edges = planned(holed.rows, HOLED_RANGES)
    assert (direct, edges) == (1 + 2 + 1 + 1, 7) and counters == {"decoded": decoded, "direct": direct, "rounds": 1}
    st, res, small, got = read(mods, holed, holed.rows, HOLED_RANGES, scratch=128 * KiB)         # two edge slots a round
    check_clean(holed, HOLED_RANGES, st, res, got)
    assert small["rounds"] > 1 and small["direct"] == direct and small["decoded"] >= decoded


def test_read_with_rows_of_every_source(mods, holed):
    ranges = [(0, 20000), (997 * 10 - 1, 2)]
    idx = index(mods, holed)[1]
    gz = gunzip(mods, holed)[3]
    assert idx == gz == holed.rows
    st, res, counters, got = read(mods, holed, idx, ranges)
    check_clean(holed, ranges, st, res, got)
    assert counters == {"decoded": 21 + 2, "direct": 21, "rounds": 1}
    st, res, counters, got = read(mods, holed, [], ranges)                  # no members: every range is beyond the end
    assert st == 0 and res == [(1, 0, None)] * 2 and got == [b"\xab" * 20000, b"\xab" * 2] and counters["decoded"] == 0


def test_slice_alignments(mods, big3):
    base = BGZF_BLOCK - 1504
    assert base % 16 == 0
    ranges = [(base + a, 3000) for a in range(16) for _ in range(16)]       # begins inside member 0, ends inside member 1
    odds = [b for _ in range(16) for b in range(16)]
    st, res, counters, got = read(mods, big3, big3.rows, ranges, odds)
    check_clean(big3, ranges, st, res, got)
    assert counters == {"decoded": 2, "direct": 0, "rounds": 1}
    ranges, odds = [], []
    for n in range(1, 41):                                                  # short slices at a member border, and next to it
        ranges += [(2 * BGZF_BLOCK - n // 2, n), (2 * BGZF_BLOCK - n, n), (2 * BGZF_BLOCK, n)]
        odds += [n % 16, (3 * n + 1) % 16, (16 - n) % 16]
    st, res, counters, got = read(mods, big3, big3.rows, ranges, odds)
    check_clean(big3, ranges, st, res, got)
    assert counters == {"decoded": 2, "direct": 0, "rounds": 1}


def test_whole_members_at_every_destination_alignment(mods, big3):
    ranges = [(BGZF_BLOCK, BGZF_BLOCK)] * 16 + [(0, 3 * BGZF_BLOCK)]
    st, res, counters, got = read(mods, big3, big3.rows, ranges, list(range(16)) + [9])
    check_clean(big3, ranges, st, res, got)
    assert counters == {"decoded": 19, "direct": 19, "rounds": 1}


# ---- failures ---------------------------------------------------------------------------------------------------------------
def flipped(f, k):
    """the file with one payload bit of member k changed so that the member still decodes to as many bytes, but other ones:
    (bytes, CPython's message -- the check value's)"""
    off, used, _, out_len = f.rows[k][:4]
    for at in range(off + 18 + (used - 26) // 2, off + used - 8):
        for bit in range(8):
            bad = bytearray(f.data)
            bad[at] ^= 1 << bit
            d = zlib.decompressobj(-15)
            try:
                out = d.decompress(bytes(bad[off + 18:off + used - 8]))
            except zlib.error:
                continue
            if not d.eof or d.unused_data or len(out) != out_len:
                continue
            try:
                zlib.decompressobj(31).decompress(bytes(bad[off:off + used]))
            except zlib.error as e:
                assert "Error -3" in str(e)
                return bytes(bad), str(e).split(": ", 1)[1]
    raise AssertionError("no flip kept the length")


def test_failure_isolation(mods, tiny):
    k = 5                                                                   # plaintext [4985, 5982)
    bad, text = flipped(tiny, k)
    f = File(mods, bad, odd=9, oracle=False)
    ranges = [(0, 2000),            # does not touch k
              (5000, 2000),         # k is the first edge; member 6 whole and an edge of 7 behind it
              (4000, 1500),         # edge 4, then k as the last edge
              (4500, 2000),         # edge 4, k interior, edge 6
              (5982, 100),          # begins where k ends
              (5100, 10)]           # inside k
    st, res, counters, got = read(mods, f, tiny.rows, ranges)
    assert st == 0
    plain = tiny.plain
    assert res[0] == (1, 2000, None) and got[0] == plain[:2000]
    assert res[4] == (1, 100, None) and got[4] == plain[5982:6082]
    assert res[1] == (DATA_ERROR, 0, text)
    assert got[1][:982] == b"\xab" * 982 and got[1][982:] == plain[5982:7000]          # k's slice delivered nothing
    assert res[2] == (DATA_ERROR, 985, text)
    assert got[2] == plain[4000:4985] + b"\xab" * 515
    assert res[3] == (DATA_ERROR, 485, text)                                # (Arena.check: nothing outside its len bytes)
    assert got[3][:485] == plain[4500:4985] and got[3][485 + 997:] == plain[5982:6500]
    assert res[5] == (DATA_ERROR, 0, text) and got[5] == b"\xab" * 10
    assert counters["rounds"] == 1


def test_stale_index(mods, tiny):
    for j, delta in ((7, 1), (7, -1)):
        rows = [list(r) for r in tiny.rows]
        rows[j][3] += delta
        for r in rows[j + 1:]:
            r[2] += delta                                                   # dst_off stays contiguous
        rows = [tuple(r) for r in rows]
        lo = rows[j][2]
        ranges = [(0, lo),                      # in front of row j
                  (lo + 10, 100),               # row j as an edge
                  (lo - 10, 20)]                # the edge in front, and row j cut
        if delta > 0:
            ranges.append((lo - 5, rows[j][3] + 10))                        # row j interior: one byte more room than it fills
        st, res, counters, got = read(mods, tiny, rows, ranges)
        assert st == 0 and res[0] == (1, lo, None) and got[0] == tiny.plain[:lo]
        assert res[1] == (DATA_ERROR, 0, ROW_MSG) and got[1] == b"\xab" * 100
        assert res[2] == (DATA_ERROR, 10, ROW_MSG) and got[2] == tiny.plain[lo - 10:lo] + b"\xab" * 10
        if delta > 0:
            assert res[3] == (DATA_ERROR, 5, ROW_MSG) and got[3][:5] == tiny.plain[lo - 5:lo]


def test_truncated_file_with_the_whole_index_is_refused(mods, tiny):
    last = tiny.rows[-2]
    f = File(mods, tiny.data[:last[0] + last[1] // 2], oracle=False)
    st, res, counters, got = read(mods, f, tiny.rows, [(0, 100), (19990, 10)])
    assert st == EINVAL and res == [(0, 0, None)] * 2 and got == [b"\xab" * 100, b"\xab" * 10]
    assert counters == {"decoded": 0, "direct": 0, "rounds": 0}


def test_refusals_leave_everything_untouched(mods, tiny):
    torch, _, inf, zr = mods
    lib = zr.rocm.lib()
    good = tiny.rows

    def edit(k, field, value):
        rows = [list(r) for r in good]
        rows[k][field] = value
        return [tuple(r) for r in rows]
    cases = [(edit(3, 0, good[2][0]), 0, "order"), (edit(3, 0, good[3][0] - 1), 0, "overlap"), (edit(21, 0, len(tiny.data) - 27), 0, "outside"),
             (edit(0, 2, 1), 0, "dst_off from 0"), (edit(4, 2, good[4][2] + 1), 0, "dst_off contiguous"), (edit(6, 5, 0), 0, "bgzf"),
             (edit(21, 1, 27), 0, "src_len below 28"), (edit(2, 1, 65537), 0, "src_len above 65536"), (edit(2, 3, 65537), 0, "out_len"),
             (good, 1000, "scratch below 128 KiB"), (good, 128 * KiB - 1, "scratch below 128 KiB"), (good, (4 << 30) + 1, "scratch above 4 GiB")]
    arena = Arena(torch, [(0, 3000), (5000, 10)])
    for rows, scratch, note in cases + [(good, 0, "null d_dst")]:
        rs = (inf.BgzfRange * 2)(inf.BgzfRange(0, 3000, arena.ptrs[0], 77, 77, b"mine"),
                                 inf.BgzfRange(5000, 10, None if note == "null d_dst" else arena.ptrs[1], 77, 77, b"mine"))
        st = lib.zng_rocm_bgzf_read_dev(tiny.src.data_ptr(), len(tiny.data), C.cast(inf.member_table(rows), C.c_void_p), len(rows),
                                        C.cast(rs, C.c_void_p), 2, scratch, None)
        assert st == EINVAL, note
        assert all((r.status, r.out_len, r.msg) == (77, 77, b"mine") for r in rs), note
        assert arena.check() == [b"\xab" * 3000, b"\xab" * 10], note
    rs = (inf.BgzfRange * 1)(inf.BgzfRange(0, 0, None, 77, 77, None))       # a null d_dst with len 0 is no refusal
    assert lib.zng_rocm_bgzf_read_dev(tiny.src.data_ptr(), len(tiny.data), C.cast(inf.member_table(good), C.c_void_p), len(good),
                                      C.cast(rs, C.c_void_p), 1, 0, None) == 0 and (rs[0].status, rs[0].out_len) == (1, 0)


# ---- with the writer --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(level=6), dict(level=1, quick=True)])
def test_round_trip_with_the_writer(mods, lcet, kw):
    torch, dfl, inf, _ = mods
    plain = lcet[:3 * BGZF_BLOCK + 4321]
    src = place(torch, plain, 5)
    whole = torch.zeros(16 + dfl.bgzf_bound(len(plain), 0), dtype=torch.uint8, device="cuda")
    st, out_len, rows, nmembers, _ = dfl.bgzf_compress_dev(src, whole[3:], **kw)
    torch.cuda.synchronize()
    assert st == 0 and nmembers == len(rows) == 5

    class Written:
        pass
    f = Written()
    f.src, f.plain, f.rows = whole[3:3 + out_len], plain, rows
    ranges = [(0, 100), (BGZF_BLOCK - 50, 100), (BGZF_BLOCK, BGZF_BLOCK), (100000, 100000), (len(plain) - 7, 100), (0, len(plain))]
    st, res, counters, got = read(mods, f, rows, ranges)
    check_clean(f, ranges, st, res, got)
    decoded, direct, _ = planned(rows, ranges)
    assert counters == {"decoded": decoded, "direct": direct, "rounds": 1}
    ist, irows, inm, iplain, iused = inf.bgzf_index_dev(f.src)
    assert (ist, inm, iplain, iused) == (0, 5, len(plain), out_len) and irows == rows


# ---- virtual offsets through the library ------------------------------------------------------------------------------------
def test_virtual_offsets(mods, holed):
    _, _, inf, _ = mods
    rows = holed.rows
    table = inf.member_table(rows)
    for u in (0, 1, 996, 997, 9969, 9970, 9971, 19999):
        holder, = [r for r in rows if r[2] <= u < r[2] + r[3]]
        v = inf.bgzf_voffset(table, u)
        assert v == (holder[0] << 16) | (u - holder[2]) and inf.bgzf_uoffset(table, v) == u
    assert inf.bgzf_voffset(rows, 9970) == rows[11][0] << 16                # behind the empty member: the next non-empty one
    assert inf.bgzf_voffset(rows, 20000) == rows[-1][0] << 16 and inf.bgzf_voffset(rows, 20001) is None
    assert inf.bgzf_uoffset(rows, (rows[3][0] << 16) | 997) == 4 * 997 and inf.bgzf_uoffset(rows, (rows[3][0] << 16) | 998) is None
    assert inf.bgzf_uoffset(rows, (rows[3][0] + 1) << 16) is None and inf.bgzf_uoffset(rows, (rows[10][0] << 16) | 1) is None
