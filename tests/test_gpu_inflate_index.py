"""Random access into plain deflate, zlib and gzip streams on the device, through the C ABI: zng_rocm_inflate_index_build_dev
(zng_rocm_uncompress_large_dev plus the access points), zng_rocm_inflate_index_read_dev (many plaintext ranges in one set of
launches), export and import.
Oracle for an access point, independent of the library: drop in_bit bits from the file, decode what is left with CPython's
zlib.decompressobj(-15, zdict=window): it must give plain[out_off:].  Oracle for a read: Python slicing.  Every destination sits
at a chosen address modulo 16 inside one arena of 0xAB with guard bytes on both sides, and the whole arena is compared with the
one built here, so a byte written outside a destination fails the test that wrote it."""
import importlib
import struct
import zlib

import numpy as np
import pytest

import synth
from wrapped_members import place

pytestmark = pytest.mark.gpu
EINVAL, DATA_ERROR, BUF_ERROR = -3, -3, -5
KiB, MiB = 1 << 10, 1 << 20
WBITS = {0: -15, 1: 15, 2: 31}
LENGTHS = (0, 1, 15, 16, 17, 4095, 65536, 300000)
HEAD, ROW = 56, 24


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), zr, importlib.import_module("zlib-ng_amd.oneshot")


# ---- streams ----------------------------------------------------------------------------------------------------------------
def flushed(plain, fmt, every, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, cuts=None):
    """the stream with Z_SYNC_FLUSH behind every `every` bytes of input (or at `cuts`), and the markers [(byte, out_off)]: a
    block starts at byte `byte` of the file, byte aligned, with out_off bytes of plaintext in front of it"""
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt], 8, strategy)
    cuts = list(range(every, len(plain), every)) if cuts is None else cuts
    out, marks, at = [], [], 0
    for cut in cuts:
        out.append(c.compress(plain[at:cut]) + c.flush(zlib.Z_SYNC_FLUSH))
        at = cut
        marks.append((sum(len(o) for o in out), cut))
    out.append(c.compress(plain[at:]) + c.flush())
    return b"".join(out), marks


def drop_bits(data, bit):
    """the file from bit `bit` on, repacked (what numpy.unpackbits(..., bitorder='little')[bit:] repacked gives)"""
    a = np.frombuffer(data, dtype=np.uint8)[bit >> 3:]
    s = bit & 7
    if not s:
        return a.tobytes()
    nxt = np.concatenate([a[1:], np.zeros(1, dtype=np.uint8)])
    return ((a >> s) | (nxt << (8 - s))).astype(np.uint8).tobytes()


def test_drop_bits_is_the_unpackbits_round_trip():
    data = bytes(range(256)) * 3
    for bit in (0, 1, 7, 8, 13, 100):
        bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8), bitorder="little")[bit:]
        assert drop_bits(data, bit) == np.packbits(bits, bitorder="little").tobytes()


def check_points(data, plain, pts, header_len, windows=None, only=None):
    """point 0 as specified, strictly ascending, windows as specified, and every point decodes the rest of the plaintext"""
    assert pts[0] == (8 * header_len, 0, 0)
    for k, (in_bit, out_off, wl) in enumerate(pts):
        if k:
            assert in_bit > pts[k - 1][0] and out_off > pts[k - 1][1]
        assert wl == min(32768, out_off) and out_off < max(len(plain), 1)
        window = plain[out_off - wl:out_off]
        if windows is not None:
            assert windows[k] == window, k
        if only is not None and not only(k, in_bit, out_off):
            continue
        d = zlib.decompressobj(-15, zdict=window) if wl else zlib.decompressobj(-15)
        assert d.decompress(drop_bits(data, in_bit)) == plain[out_off:], (k, in_bit, out_off)
        assert d.eof


def blob_windows(blob):
    n = struct.unpack_from("<Q", blob, 48)[0]
    rows = [struct.unpack_from("<QQII", blob, HEAD + ROW * k) for k in range(n)]
    at, out = HEAD + ROW * n, []
    for _, _, wl, _ in rows:
        out.append(blob[at:at + wl])
        at += wl
    assert at == len(blob)
    return [r[:3] for r in rows], out


class Stream:
    """a stream in device memory at an odd address, its plaintext, and (built on demand) its index"""

    def __init__(self, mods, data, plain, fmt, odd=3):
        self.mods, self.data, self.plain, self.fmt = mods, bytes(data), bytes(plain), fmt
        self.src = place(mods[0], self.data, odd)

    def build(self, span=0, piece_bytes=0, subblock=False, cap=None, src=None):
        torch, inf, zr, _ = self.mods
        dst = torch.full((len(self.plain) + 64 if cap is None else cap,), 0xAB, dtype=torch.uint8, device="cuda")
        st, out_len, in_used, idx = inf.InflateIndex.build(self.fmt, self.src if src is None else src, dst, span_bytes=span,
                                                           piece_bytes=piece_bytes, subblock=subblock)
        lib = zr.rocm.lib()
        counters = (int(lib.zng_rocm_inflate_large_last_parts()), int(lib.zng_rocm_inflate_large_last_pieces()),
                    int(lib.zng_rocm_inflate_large_last_host_bytes()))
        return st, out_len, in_used, idx, dst, counters, lib.zng_rocm_last_error().decode()

    def whole(self, piece_bytes=0, subblock=False):
        torch, inf, zr, _ = self.mods
        dst = torch.full((len(self.plain) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        out = inf.uncompress_large_dev(self.fmt, self.src, dst, piece_bytes=piece_bytes, subblock=subblock)
        return out, dst, zr.rocm.lib().zng_rocm_last_error().decode()


def header_len(data, fmt):
    return {0: 0, 1: 2, 2: 10}[fmt]                       # (the writers here add no optional gzip field)


# ---- reads ----------------------------------------------------------------------------------------------------------------
GUARD = 48


def read_check(mods, idx, src, plain, ranges, scratch=0, src_len=None, want=None):
    """`ranges` = [(uoff, len, alignment)].  Reads them into one arena, compares the WHOLE arena with the expected one (`want`
    per range: (status, out_len, msg, bytes in place) -- default: status 1, the clipped slice) and returns the counters."""
    torch = mods[0]
    offs, at = [], 0
    for uoff, length, align in ranges:
        at = ((at + GUARD + 15) & ~15) + align
        offs.append(at)
        at += length
    arena = torch.full((at + GUARD + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    expect = np.full(arena.numel(), 0xAB, dtype=np.uint8)
    rc, out, counters = idx.read(src, [(u, n, arena.data_ptr() + o) for (u, n, _), o in zip(ranges, offs)], scratch_bytes=scratch,
                                 src_len=src_len)
    torch.cuda.synchronize()
    assert rc == 0
    for k, ((uoff, length, _), o) in enumerate(zip(ranges, offs)):
        clipped = max(0, min(length, len(plain) - uoff))
        status, out_len, msg, filled = (1, clipped, None, [(0, clipped)]) if want is None or want[k] is None else want[k]
        assert out[k] == (status, out_len, msg), (k, ranges[k], out[k])
        for lo, hi in filled:
            expect[o + lo:o + hi] = np.frombuffer(plain[uoff + lo:uoff + hi], dtype=np.uint8)
    got = arena.cpu().numpy()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, ("first differing arena byte", int(bad[0]), "of", bad.size)
    return counters


def seeded_ranges(plain_len, count, seed, lengths=LENGTHS):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        length = int(lengths[k % len(lengths)])
        kind = k % 10
        if kind == 0:
            uoff = plain_len + int(rng.integers(0, 100000))                # wholly behind the end
        elif kind == 1:
            uoff = max(0, plain_len - int(rng.integers(0, max(length, 1) + 1)))   # runs past the end: clipped
        else:
            uoff = int(rng.integers(0, plain_len))
        out.append((uoff, length, k % 16))
    return out


# ---- 1: placed flush points -------------------------------------------------------------------------------------------------
PLACED = {}


def placed(mods, fmt):
    """3 MiB of text, level 6, Z_SYNC_FLUSH every 48 KiB of input, indexed with a span of 64 KiB (built once per format)"""
    if fmt not in PLACED:
        plain = synth.silesia_like(3 * MiB, seed=0x1DE0 + fmt).tobytes()
        data, marks = flushed(plain, fmt, 48 * KiB)
        s = Stream(mods, data, plain, fmt, odd=(3, 5, 9)[fmt])
        s.marks = marks
        s.built = s.build(span=64 * KiB)
        PLACED[fmt] = s
    return PLACED[fmt]


@pytest.mark.parametrize("fmt", [0, 1, 2])
def test_placed_flush_points(mods, fmt):
    torch = mods[0]
    s = placed(mods, fmt)
    st, out_len, in_used, idx, dst, counters, err = s.built
    (wst, wout, wused, wparts, wpieces, whost), wdst, werr = s.whole()
    assert (st, out_len, in_used, err) == (wst, wout, wused, werr) and st == 1
    assert (out_len, in_used) == (len(s.plain), len(s.data))
    assert torch.equal(dst, wdst) and dst[:out_len].cpu().numpy().tobytes() == s.plain
    assert counters == (wparts, wpieces, whost) and counters[0] > 0, "the device path decoded it"
    assert idx is not None and idx.plain_len == len(s.plain)
    pts = idx.points()
    rows, windows = blob_windows(idx.save())
    assert rows == pts
    check_points(s.data, s.plain, pts, header_len(s.data, fmt), windows)
    assert all(b[1] - a[1] >= 64 * KiB for a, b in zip(pts, pts[1:]))
    # every placed flush point is a block start the finder can see: the greedy rule over them alone gives `greedy` points, and
    # the index, which thins the finder's starts further, must have at least half as many
    greedy, last = 1, 0
    for _, out_off in s.marks:
        if out_off >= last + 64 * KiB and out_off < len(s.plain):
            greedy, last = greedy + 1, out_off
    assert greedy >= 30
    assert 2 * len(pts) >= greedy, (len(pts), greedy)


# ---- 2, 3: reads and rounds ---------------------------------------------------------------------------------------------------
def test_reads(mods):
    s = placed(mods, 2)
    idx = s.built[3]
    ranges = seeded_ranges(len(s.plain), 200, seed=21)
    assert {r[2] for r in ranges} == set(range(16)) and {r[1] for r in ranges} == set(LENGTHS)
    assert any(u >= len(s.plain) for u, _, _ in ranges) and any(u < len(s.plain) < u + n for u, n, _ in ranges)
    counters = read_check(mods, idx, s.src, s.plain, ranges)
    assert counters["direct"] > 0 and counters["rounds"] == 1 and counters["decoded"] >= counters["direct"]


def test_interior_spans_and_a_shared_edge(mods):
    s = placed(mods, 2)
    idx = s.built[3]
    pts = idx.points()
    # from inside span 2 to inside span 6: spans 3, 4, 5 are interior (straight into the destination), 2 and 6 are edges
    lo, hi = pts[2][1] + 1000, pts[6][1] + 777
    counters = read_check(mods, idx, s.src, s.plain, [(lo, hi - lo, 5)])
    assert counters == {"decoded": 5, "direct": 3, "rounds": 1}
    # two ranges cut the same span: it is decoded once; a third range wants all of it: a direct job of its own
    a = pts[4][1]
    counters = read_check(mods, idx, s.src, s.plain, [(a + 10, 100, 1), (a + 5000, 3000, 9)])
    assert counters == {"decoded": 1, "direct": 0, "rounds": 1}
    counters = read_check(mods, idx, s.src, s.plain, [(a + 10, 100, 1), (a, pts[5][1] - a, 2), (a + 5000, 3000, 9)])
    assert counters == {"decoded": 2, "direct": 1, "rounds": 1}
    # no ranges, and ranges that want nothing
    assert read_check(mods, idx, s.src, s.plain, []) == {"decoded": 0, "direct": 0, "rounds": 0}
    assert read_check(mods, idx, s.src, s.plain, [(5, 0, 3), (len(s.plain), 10, 4)]) == {"decoded": 0, "direct": 0, "rounds": 0}


def test_rounds(mods):
    s = placed(mods, 2)
    ranges = seeded_ranges(len(s.plain), 200, seed=21)
    counters = read_check(mods, s.built[3], s.src, s.plain, ranges, scratch=1 * MiB)
    assert counters["rounds"] > 1 and counters["direct"] > 0


# ---- 4: streams without placed points ---------------------------------------------------------------------------------------
def cpython(plain, level, fmt, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, WBITS[fmt], 8, strategy)
    return c.compress(plain) + c.flush()


@pytest.mark.parametrize("name", ["cpython1", "cpython6", "cpython9", "device6_zlib", "device6_gzip", "fixed", "fixed_subblock"])
def test_streams_without_placed_points(mods, name):
    torch, inf, zr, one = mods
    plain = synth.silesia_like(2 * MiB + 12345, seed=0x1DE7).tobytes()
    fmt, sub = 0, False
    if name.startswith("cpython"):
        fmt = {"1": 0, "6": 1, "9": 2}[name[-1]]
        data = cpython(plain, int(name[-1]), fmt)
    elif name.startswith("device6"):
        fmt = 1 if name.endswith("zlib") else 2
        dev, n = one.compress2_dev(place(torch, plain, 0), level=6, fmt=fmt)
        data = dev[:n].cpu().numpy().tobytes()
    else:
        data, sub = cpython(plain, 6, 0, zlib.Z_FIXED), name.endswith("subblock")
    s = Stream(mods, data, plain, fmt, odd=7)
    st, out_len, in_used, idx, dst, counters, _ = s.build(span=64 * KiB, subblock=sub)
    assert (st, out_len, in_used) == (1, len(plain), len(data)) and dst[:out_len].cpu().numpy().tobytes() == plain
    pts = idx.points()
    assert len(pts) >= 1
    check_points(data, plain, pts, header_len(data, fmt))
    assert all(b[1] - a[1] >= 64 * KiB for a, b in zip(pts, pts[1:]))
    read_check(mods, idx, s.src, plain, seeded_ranges(len(plain), 50, seed=4))


# ---- 5: the sequential decoder's streams, and a short window ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "stored"])
def test_sequential_decoder_streams(mods, name):
    plain = synth.silesia_like(300 * KiB if name == "small" else 100 * KiB, seed=0x1DE9).tobytes()
    data = cpython(plain, 9 if name == "small" else 0, 2)
    assert len(data) < 128 * KiB
    s = Stream(mods, data, plain, 2, odd=11)
    st, out_len, in_used, idx, dst, counters, _ = s.build(span=64 * KiB)
    assert (st, out_len, in_used) == (1, len(plain), len(data)) and counters[0] == 0
    assert idx.points() == [(80, 0, 0)]
    c = read_check(mods, idx, s.src, plain, seeded_ranges(len(plain), 40, seed=6) + [(0, len(plain), 3)])
    assert c["direct"] >= 1


def test_short_window(mods):
    """No build gives a point with out_off below 32768 (a span is 64 KiB at least), but a saved index may hold one: here the
    flush point at plaintext byte 20000 is added to a built index's blob, with the 20000 bytes in front of it as its window."""
    torch, inf, zr, _ = mods
    plain = synth.silesia_like(300 * KiB, seed=0x1DEA).tobytes()
    data, marks = flushed(plain, 1, 0, cuts=[20000, 150000])
    s = Stream(mods, data, plain, 1, odd=13)
    st, out_len, in_used, idx, dst, counters, _ = s.build(span=64 * KiB)
    assert st == 1 and len(idx.points()) >= 1
    blob = idx.save()
    head = bytearray(blob[:HEAD])
    pts = [(16, 0, 0), (8 * marks[0][0], 20000, 20000), (8 * marks[1][0], 150000, 32768)]
    struct.pack_into("<Q", head, 48, len(pts))
    made = bytes(head) + b"".join(struct.pack("<QQII", *p, 0) for p in pts) + plain[:20000] + plain[150000 - 32768:150000]
    rc, short = inf.InflateIndex.load(made)
    assert rc == 0 and short.points() == pts
    check_points(data, plain, pts, 2)
    ranges = [(20000, 130000, 3), (19990, 100, 7), (20000 + 40000, 5000, 0), (0, len(plain), 15)] + seeded_ranges(len(plain), 30, seed=8)
    c = read_check(mods, short, s.src, plain, ranges)
    assert c["direct"] >= 4                                  # span 1 whole (its copies reach into the 20000-byte window) and all three


# ---- 6: several pieces ------------------------------------------------------------------------------------------------------
def test_several_pieces(mods):
    rng = np.random.default_rng(0x1DEB)
    text = synth.silesia_like(14 * MiB, seed=0x1DEB)
    noise = rng.integers(0, 256, size=14 * MiB, dtype=np.uint8)
    weak = np.where((np.arange(14 * MiB) % (256 * KiB)) < 170 * KiB, noise, text).astype(np.uint8).tobytes()
    data, marks = flushed(weak, 2, 256 * KiB)
    assert len(data) > 8 * MiB
    s = Stream(mods, data, weak, 2, odd=1)
    st, out_len, in_used, idx, dst, counters, _ = s.build(span=1 * MiB, piece_bytes=4 * MiB)
    assert (st, out_len, in_used) == (1, len(weak), len(data)) and counters[1] >= 2
    assert dst[:out_len].cpu().numpy().tobytes() == weak
    pts = idx.points()
    behind = [p for p in pts if (p[0] >> 3) > 4 * MiB]
    assert len(behind) >= 3, "points behind the first piece: the later passes' base offsets reached the index"
    check_points(data, weak, pts, 10, only=lambda k, in_bit, out_off: k == 0 or (in_bit >> 3) > 4 * MiB)
    assert all(b[1] - a[1] >= 1 * MiB for a, b in zip(pts, pts[1:]))
    # ranges across every point (piece boundaries are among them or between them), and long ones across the whole file
    ranges = [(p[1] - 3000, 70000, k % 16) for k, p in enumerate(pts[1:])] + [(k * 3 * MiB + 17, 3 * MiB + 50000, k) for k in range(5)]
    c = read_check(mods, idx, s.src, weak, ranges)
    assert c["direct"] > 0


# ---- 7: damage and refusals -------------------------------------------------------------------------------------------------
def test_truncated_file(mods):
    s = placed(mods, 2)
    idx = s.built[3]
    pts = idx.points()
    n, last = len(s.plain), pts[-1]
    cut = ((last[0] >> 3) + len(s.data)) // 2               # inside the last span: every point still begins inside the file
    ranges = [(n - 1000, 1000, 3),                          # the end of the cut span: starved
              (last[1] - 5000, n - 1 - (last[1] - 5000), 6),     # from the span in front into the cut one: the bytes in front are in place
              (pts[-3][1] + 7, pts[-2][1] - pts[-3][1] + 100, 9),       # spans in front of the cut: untouched by it
              (100, 300000, 12)]
    want = [(BUF_ERROR, 0, None, []), (BUF_ERROR, 5000, None, [(0, 5000)]), None, None]
    read_check(mods, idx, s.src, s.plain, ranges, src_len=cut, want=want)
    # a file that ends in front of the last point is not the indexed one
    rc, out, _ = idx.read(s.src, [(0, 10, None)], src_len=last[0] >> 3)
    assert rc == EINVAL and out == [(0, 0, None)]


def test_corrupted_span(mods):
    torch = mods[0]
    s = placed(mods, 1)
    idx = s.built[3]
    pts = idx.points()
    # a point on a byte boundary (the flush points are): the span in front of it then ends in front of the damaged bytes
    k = next(i for i in range(len(pts) // 2, len(pts) - 3) if pts[i][0] % 8 == 0)
    bad = bytearray(s.data)
    bad[pts[k][0] >> 3:(pts[k][0] >> 3) + 2] = b"\xff\xff"
    src = place(torch, bytes(bad), 3)
    a, b = pts[k][1], pts[k + 1][1]
    ranges = [(a + 100, 2000, 5),                            # begins in the damaged span, an edge: nothing is written
              (a, b - a, 2),                                 # the damaged span whole, a direct job: status says so
              (pts[k - 1][1] - 4000, a + 500 - (pts[k - 1][1] - 4000), 7),     # two good spans, then the damaged one
              (pts[k - 3][1] + 5, pts[k - 2][1] - pts[k - 3][1], 11),         # two and more spans away: fine
              (pts[k + 2][1] + 5, 200000, 14)]
    third_front = a - (pts[k - 1][1] - 4000)
    want = [(DATA_ERROR, 0, "invalid block type", []), (DATA_ERROR, 0, "invalid block type", None),
            (DATA_ERROR, third_front, "invalid block type", None), None, None]
    # (what a failed DIRECT job leaves inside its own destination is not specified: those ranges are read apart, below)
    read_check(mods, idx, src, s.plain, [ranges[0], ranges[3], ranges[4]], want=[want[0], None, None])
    rc, out, _ = idx.read(src, [(u, n, torch.zeros(n + 16, dtype=torch.uint8, device="cuda")) for u, n, _ in ranges[1:3]])
    assert rc == 0 and out == [want[1][:3], want[2][:3]]


def test_refusals(mods):
    torch, inf, zr, _ = mods
    s = placed(mods, 2)
    idx = s.built[3]
    for span in (1, 64 * KiB - 1, (1 << 30) + 1):
        st, out_len, in_used, none, dst, _, err = s.build(span=span)
        assert (st, out_len, in_used, none) == (EINVAL, 0, 0, None) and "span_bytes" in err
        assert bool((dst == 0xAB).all()), "nothing launched or written"
    dst = torch.full((4096,), 0xAB, dtype=torch.uint8, device="cuda")
    good = (100, 1000, dst)
    for kw, ranges in (({"scratch_bytes": 4096}, [good]), ({"scratch_bytes": (4 << 30) + 1}, [good]), ({}, [good, (5, 10, None)]),
                       ({"src_len": 1000}, [good])):
        rc, out, _ = idx.read(s.src, ranges, **kw)
        assert rc == EINVAL and all(o == (0, 0, None) for o in out), (kw, out)
        assert bool((dst == 0xAB).all())
    rc, out, _ = idx.read(s.src, [(5, 0, None), good])      # a null destination with no length is no violation
    assert rc == 0 and out == [(1, 0, None), (1, 1000, None)] and dst[:1000].cpu().numpy().tobytes() == s.plain[100:1100]


def test_fdict_and_two_members(mods):
    torch, inf, zr, _ = mods
    plain = synth.silesia_like(300 * KiB, seed=0x1DEC).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_DEFAULT_STRATEGY, plain[:1000])
    s = Stream(mods, c.compress(plain) + c.flush(), plain, 1)
    st, out_len, in_used, idx, dst, _, _ = s.build()
    (wst, wout, wused, _, _, _), _, _ = s.whole()
    assert (st, out_len, in_used) == (wst, wout, wused) and st == 2 and idx is None
    a, b = cpython(plain, 6, 2), cpython(plain[::-1], 6, 2)
    two = Stream(mods, a + b, plain, 2, odd=9)
    st, out_len, in_used, idx, dst, _, _ = two.build(span=64 * KiB)
    assert (st, out_len, in_used) == (1, len(plain), len(a)) and idx.plain_len == len(plain)
    blob = idx.save()
    assert struct.unpack_from("<4sIII5Q", blob)[:8] == (b"ZRIX", 1, 2, 0, 10, len(a), len(plain), 64 * KiB)
    read_check(mods, idx, two.src, plain, [(len(plain) - 50, 100, 3), (len(plain), 5, 4), (1000, 100000, 8)])


# ---- 8: export and import ---------------------------------------------------------------------------------------------------
def test_export_import(mods):
    torch, inf, zr, _ = mods
    s = placed(mods, 0)
    st, out_len, in_used, idx, dst, _, _ = s.build(span=64 * KiB)       # (an index of its own: it is destroyed here)
    pts, blob = idx.points(), idx.save()
    lib = zr.rocm.lib()
    import ctypes as C
    need = C.c_size_t(0)
    small = (C.c_uint8 * 100)(*([0xAB] * 100))
    assert lib.zng_rocm_inflate_index_export(idx._h, small, 100, C.byref(need), None) == BUF_ERROR and need.value == len(blob)
    assert bytes(small) == b"\xab" * 100
    idx.close()
    rc, back = inf.InflateIndex.load(blob)
    assert rc == 0 and back.points() == pts and back.plain_len == len(s.plain) and back.save() == blob
    ranges = seeded_ranges(len(s.plain), 200, seed=21)
    c = read_check(mods, back, s.src, s.plain, ranges)
    assert c["direct"] > 0
    changed = bytearray(blob)
    struct.pack_into("<I", changed, HEAD + ROW * 3 + 16, 32767)                # one row's window_len: not min(32768, out_off)
    swapped = bytearray(blob)
    struct.pack_into("<Q", swapped, HEAD + ROW * 3, pts[2][0])                 # one row's in_bit: no longer ascending
    wrong_version = bytearray(blob)
    struct.pack_into("<I", wrong_version, 4, 2)
    for bad in (blob[:-1], blob[:HEAD + 10], bytes(changed), bytes(swapped), bytes(wrong_version), b""):
        rc, none = inf.InflateIndex.load(bad)
        assert rc == EINVAL and none is None
    back.close()
