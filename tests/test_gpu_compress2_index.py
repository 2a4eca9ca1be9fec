"""zng_rocm_compress2_index_dev on the device, through the C ABI: compress2_dev that hands back a zng_rocm_inflate_index of the
stream it writes, taken from the compressor's own block table -- no byte of the stream is decoded to make it.

  1  the stream is compress2_dev's, byte for byte
  2  every point of the index decodes the rest of the file (CPython's zlib from bit in_bit with the window from the exported blob)
  3  the points are index_select over EVERY block start of the stream (read off the stream by tests/deflate_parse.py), and every
     span, the last one up to the end, is shorter than span_bytes + 65536
  4  reads through the index give the Python slice at all 16 destination alignments, before and after export -> import
  5  what the decode-built index cannot do: 4 MiB that compress below 128 KiB get one point from the build, many from here
  6  refusals
  7  an index of point 0 alone reads correctly
Oracles: tests/compress_index_util.py."""
import ctypes as C
import importlib

import numpy as np
import pytest

from compress_index_util import (HEADER_LEN, INPUTS, KiB, MiB, blob_head, blob_windows, block_starts, check_points, read_check, select,
                                 span_bound_holds)

pytestmark = pytest.mark.gpu
EINVAL, STREAM_ERROR, BUF_ERROR = -3, -2, -5
SMALL = (0, 1, 61439, 61440, 61441, 131071, 131072, 131073)
MULTI, BIG = 393216 + 7, 2 * MiB + 3           # three 128 KiB segments and a bit; 17 segments
STEP = 61440 + 257
NAMES = ("periodic", "texty", "random")


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), zr, importlib.import_module("zlib-ng_amd.oneshot")


FULL, MADE = {}, {}


def plain_of(name, n):
    """the first n bytes of 4 MiB of the named input (made once)"""
    if name not in FULL:
        FULL[name] = INPUTS[name](4 * MiB)
    return FULL[name][:n]


class Made:
    """one call: the plaintext on the device, the stream (device and host), the index with its points, blob and windows"""

    def __init__(self, mods, name, n, level, fmt, span):
        torch, _, _, one = mods
        self.plain, self.fmt, self.level, self.span = plain_of(name, n), fmt, level, span
        self.dev_plain = torch.from_numpy(np.frombuffer(self.plain, dtype=np.uint8).copy()).cuda() if n else \
            torch.zeros(0, dtype=torch.uint8, device="cuda")
        dst, clen, self.idx = one.compress2_index_dev(self.dev_plain, level=level, fmt=fmt, span_bytes=span)
        self.src = dst[:clen]
        self.data = self.src.cpu().numpy().tobytes()
        self.pts = self.idx.points()
        self.blob = self.idx.save()


def made(mods, name, n, level, fmt, span=64 * KiB):
    key = (name, n, level, fmt, span)
    if key not in MADE:
        MADE[key] = Made(mods, *key)
    return MADE[key]


def check_index(m):
    """head, rows and windows of the exported blob, and every point against CPython's zlib"""
    rows, windows = blob_windows(m.blob)
    assert rows == m.pts and m.idx.plain_len == len(m.plain)
    assert blob_head(m.blob) == (b"ZRIX", 1, m.fmt, 0, HEADER_LEN[m.fmt], len(m.data), len(m.plain), m.span or 1 * MiB, len(m.pts))
    check_points(m.data, m.plain, m.pts, HEADER_LEN[m.fmt], windows)


# ---- 1: the stream ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_stream_bytes_are_compress2_devs(mods, name):
    torch, _, _, one = mods
    for fmt in (0, 1, 2):
        for level in (-1, 0, 1, 6, 9):
            m = made(mods, name, MULTI, level, fmt)
            dst, clen = one.compress2_dev(m.dev_plain, level=level, fmt=fmt)
            assert clen == len(m.data) and dst[:clen].cpu().numpy().tobytes() == m.data, (fmt, level)


# ---- 2: every point -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_every_point_decodes_the_rest(mods, name):
    for fmt in (0, 1, 2):
        for level in (0, 1, 6):
            m = made(mods, name, BIG, level, fmt)
            check_index(m)
            assert len(m.pts) >= 16, (fmt, level, len(m.pts))          # 2 MiB at a span of 64 KiB + at most 65535


@pytest.mark.parametrize("name", NAMES)
def test_every_point_at_the_small_lengths(mods, name):
    for n in SMALL:
        check_index(made(mods, name, n, 6, 2))


# ---- 3: selection and the span bound --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_points_are_index_select_over_every_block_start(mods, name):
    cases = [(MULTI, level, 2) for level in (0, 1, 6)] + [(n, 6, 2) for n in SMALL] + [(MULTI, 6, 0), (MULTI, 6, 1)]
    straddled = 0
    for n, level, fmt in cases:
        m = made(mods, name, n, level, fmt)
        cands = block_starts(m.data, fmt, level)
        assert cands[0] == (8 * HEADER_LEN[fmt], 0)
        assert all(b[1] - a[1] <= (65535 if level == 0 else STEP) for a, b in zip(cands, cands[1:])), "the spacing the bound rests on"
        assert n - cands[-1][1] <= (65535 if level == 0 else 61440)
        straddled += sum(1 for _, out_off in cands if level and out_off % 1024)
        for span in (64 * KiB, 256 * KiB):
            got = made(mods, name, n, level, fmt, span)
            assert got.data == m.data
            assert got.pts == select(cands, span, n, HEADER_LEN[fmt]), (n, level, fmt, span)
            assert span_bound_holds(got.pts, n, span)
            if n < span:
                assert len(got.pts) == 1
        if n == 0:
            assert m.pts == [(8 * HEADER_LEN[fmt], 0, 0)]
    if name == "periodic":
        assert straddled > 0, "a block whose first byte is not its first position: a match straddles the border"


@pytest.mark.parametrize("name", NAMES)
def test_span_bound(mods, name):
    for level in (0, 1, 6):
        for span in (64 * KiB, 256 * KiB):
            m = made(mods, name, BIG, level, 2, span)
            assert span_bound_holds(m.pts, BIG, span), (level, span)
            assert all(b[1] - a[1] >= span for a, b in zip(m.pts, m.pts[1:]))
            assert len(m.pts) >= BIG // (span + 65536)


# ---- 4: reads -------------------------------------------------------------------------------------------------------------------
def ranges_for(pts, n, seed):
    rng = np.random.default_rng(seed)
    out = [(p[1] - 3000, 7000, k % 16) for k, p in enumerate(pts[1:])]                      # across every point
    out += [(0, 100, 1), (0, 0, 2), (n - 1000, 1000, 3), (n - 10, 100, 4), (n, 10, 5), (n + 5000, 10, 6), (5, 0, 7),
            (pts[2][1], pts[3][1] - pts[2][1], 8),                                          # one span exactly
            (pts[1][1] + 17, pts[5][1] - pts[1][1], 9),                                     # edges with interior spans between
            (0, n, 15)]
    for k in range(32):
        length = (0, 1, 15, 16, 17, 4095, 65536, 300000)[k % 8]
        out.append((int(rng.integers(0, n)), length, k % 16))
    assert {r[2] for r in out} == set(range(16))
    return out


@pytest.mark.parametrize("name,level", [("texty", 6), ("periodic", 6), ("random", 6), ("texty", 0), ("texty", 1)])
def test_reads_before_and_after_export_import(mods, name, level):
    torch, inf, _, _ = mods
    m = made(mods, name, BIG, level, 2)
    ranges = ranges_for(m.pts, BIG, seed=level)
    c = read_check(torch, m.idx, m.src, m.plain, ranges)
    assert c["direct"] > 0 and c["decoded"] >= c["direct"] and c["rounds"] == 1
    rc, back = inf.InflateIndex.load(m.blob)
    assert rc == 0 and back.points() == m.pts and back.plain_len == BIG and back.save() == m.blob
    assert read_check(torch, back, m.src, m.plain, ranges) == c
    back.close()


# ---- 5: what the decode-built index cannot do -------------------------------------------------------------------------------------
def test_bounded_spans_where_the_decode_built_index_has_one_point(mods):
    torch, inf, _, _ = mods
    n = 4 * MiB
    m = made(mods, "periodic", n, 6, 2)
    assert len(m.data) < 128 * KiB, len(m.data)
    dst = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
    st, out_len, in_used, built = inf.InflateIndex.build(2, m.src, dst, span_bytes=64 * KiB)
    assert (st, out_len, in_used) == (1, n, len(m.data)) and len(built.points()) == 1
    assert len(m.pts) >= 32 and span_bound_holds(m.pts, n, 64 * KiB)
    c = read_check(torch, m.idx, m.src, m.plain, [(n - 1000, 1000, 5)])
    assert c["decoded"] <= 2, c
    c = read_check(torch, built, m.src, m.plain, [(n - 1000, 1000, 5)])
    assert c["decoded"] == 1, "from the start of the file"
    built.close()


# ---- 6: refusals ------------------------------------------------------------------------------------------------------------------
def raw_call(mods, dev_plain, n, dst, dst_len, level, fmt, span, want_out=True):
    lib = mods[2].rocm.lib()
    dlen, h = C.c_size_t(dst_len), C.c_void_p(0xdead)
    rc = lib.zng_rocm_compress2_index_dev(C.c_void_p(dst.data_ptr()), C.byref(dlen), C.c_void_p(dev_plain.data_ptr()), n, level, fmt,
                                          span, C.byref(h) if want_out else None, None)
    mods[0].cuda.synchronize()
    return rc, dlen.value, h.value, lib.zng_rocm_last_error().decode()


def test_refusals(mods):
    torch, _, _, one = mods
    n = 100000
    m = made(mods, "texty", n, 6, 2)
    cap = one.compress_bound(n, 2)
    dst = torch.full((cap,), 0xAB, dtype=torch.uint8, device="cuda")
    for span in (1, 65535, (1 << 30) + 1):
        rc, dlen, h, err = raw_call(mods, m.dev_plain, n, dst, cap, 6, 2, span)
        assert (rc, dlen, h) == (EINVAL, cap, None) and "span_bytes" in err, span
        # before every other check: a level and a size that would be refused too
        rc, dlen, h, _ = raw_call(mods, m.dev_plain, n, dst, 5, 10, 2, span)
        assert (rc, dlen, h) == (EINVAL, 5, None)
    rc, dlen, h, err = raw_call(mods, m.dev_plain, n, dst, cap, 6, 2, 64 * KiB, want_out=False)
    assert (rc, dlen) == (EINVAL, cap) and "span_bytes" in err
    assert bool((dst == 0xAB).all()), "nothing launched or written"
    # compress2_dev's answers, with its texts, and no index
    lib = mods[2].rocm.lib()
    for dst_len, level, want in ((cap - 1, 6, BUF_ERROR), (cap, 10, STREAM_ERROR), (cap, -2, STREAM_ERROR)):
        rc, dlen, h, err = raw_call(mods, m.dev_plain, n, dst, dst_len, level, 2, 64 * KiB)
        assert (rc, dlen, h) == (want, dst_len, None)
        plain_len = C.c_size_t(dst_len)
        assert lib.zng_rocm_compress2_dev(C.c_void_p(dst.data_ptr()), C.byref(plain_len), C.c_void_p(m.dev_plain.data_ptr()), n, level, 2,
                                          None) == want
        assert lib.zng_rocm_last_error().decode() == err and err
    assert bool((dst == 0xAB).all())
    # and the accepted call into the same buffer
    rc, dlen, h, _ = raw_call(mods, m.dev_plain, n, dst, cap, 6, 2, 64 * KiB)
    assert rc == 0 and dlen == len(m.data) and h and dst[:dlen].cpu().numpy().tobytes() == m.data
    mods[1].InflateIndex(h).close()


# ---- 7: point 0 alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", (0, 6))
def test_single_point_index_reads(mods, level):
    torch = mods[0]
    for n in (0, 1, 61441):
        m = made(mods, "texty", n, level, 2)
        assert m.pts == [(80, 0, 0)]
        ranges = [(0, n, 3), (0, 10, 0), (max(n - 10, 0), 100, 9), (n, 5, 4), (n // 2, 0, 7), (n // 3, n // 2, 13)]
        c = read_check(torch, m.idx, m.src, m.plain, ranges)
        assert (c["decoded"] >= 1) == (n > 0) and c["rounds"] == (1 if n else 0)
