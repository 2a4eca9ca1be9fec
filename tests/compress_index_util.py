"""Oracles for the tests of zng_rocm_compress2_index_dev (tests/test_gpu_compress2_index.py, tests/test_deflate_index_plan_cpu.py),
independent of the library:

  drop_bits / check_points   an access point is right when the file from bit in_bit on, decoded by CPython's
                             zlib.decompressobj(-15, zdict=window), gives plain[out_off:]
  blob_windows               the rows and the windows of an exported index
  read_check                 a read is right when every range is the Python slice: every destination sits at a chosen address
                             modulo 16 inside one arena of 0xAB with guard bytes on both sides, and the WHOLE arena is compared
  block_starts               the block starts of a deflate stream of byte-aligned blocks, found by decoding it block by block
  select / span_bound        index_select and the span bound, restated
  the inputs                 periodic, texty, random"""
import struct
import zlib

import numpy as np

import deflate_parse
import synth

KiB, MiB = 1 << 10, 1 << 20
HEAD, ROW = 56, 24
GUARD = 48
HEADER_LEN = {0: 0, 1: 2, 2: 10}
TRAILER_LEN = {0: 0, 1: 4, 2: 8}
SLACK = 65536


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def periodic(n, seed=7):
    """a 300-byte period with a random edit about every 5000 bytes: long matches straddle nearly every block border"""
    rng = np.random.default_rng(seed)
    period = rng.integers(0, 256, size=300, dtype=np.uint8)
    a = np.tile(period, n // 300 + 1)[:n].copy()
    at = 0
    while True:
        at += int(rng.integers(2500, 7500))
        if at >= n:
            break
        a[at] = (int(a[at]) + 1 + int(rng.integers(0, 255))) & 0xff
    return a.tobytes()


def texty(n, seed=11):
    return synth.silesia_like(n, seed=seed).tobytes() if n else b""


def random_bytes(n, seed=13):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


INPUTS = {"periodic": periodic, "texty": texty, "random": random_bytes}


# ---- points -------------------------------------------------------------------------------------------------------------------
def drop_bits(data, bit):
    """the file from bit `bit` on, repacked (what numpy.unpackbits(..., bitorder='little')[bit:] repacked gives)"""
    a = np.frombuffer(data, dtype=np.uint8)[bit >> 3:]
    s = bit & 7
    if not s:
        return a.tobytes()
    nxt = np.concatenate([a[1:], np.zeros(1, dtype=np.uint8)])
    return ((a >> s) | (nxt << (8 - s))).astype(np.uint8).tobytes()


def check_points(data, plain, pts, header_len, windows=None):
    """point 0 as specified, strictly ascending, windows as specified, and EVERY point decodes the rest of the plaintext"""
    assert pts[0] == (8 * header_len, 0, 0)
    for k, (in_bit, out_off, wl) in enumerate(pts):
        if k:
            assert in_bit > pts[k - 1][0] and out_off > pts[k - 1][1]
        assert wl == min(32768, out_off) and out_off < max(len(plain), 1)
        window = plain[out_off - wl:out_off]
        if windows is not None:
            assert windows[k] == window, k
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


def blob_head(blob):
    """(magic, version, format, 0, header_len, src_end, plain_len, span_bytes, npoints)"""
    return struct.unpack_from("<4sIII5Q", blob)


# ---- the candidates, from the stream itself -----------------------------------------------------------------------------------
def block_starts(data, fmt, level):
    """[(bit of the file, plaintext offset)] of every block the compressor wrote, in stream order, read off the stream itself by
    the independent parser (tests/deflate_parse.py).  Level 0: every stored block.  Levels 1..9: a block of the rows engine is
    either one stored block or a static / dynamic block followed by the empty stored block that brings it to a byte boundary;
    behind the last one stands the final empty static block."""
    hl = HEADER_LEN[fmt]
    blocks = deflate_parse.parse(data[hl:len(data) - TRAILER_LEN[fmt]]).blocks
    if level == 0:
        assert all(b.btype == deflate_parse.STORED for b in blocks) and blocks[-1].final
        return [(8 * hl + b.start, b.out_start) for b in blocks]
    assert blocks[-1].final and blocks[-1].btype == deflate_parse.STATIC and blocks[-1].nbytes == 0
    out, i = [], 0
    while i < len(blocks) - 1:
        b = blocks[i]
        assert b.start % 8 == 0 and not b.final
        out.append((8 * hl + b.start, b.out_start))
        if b.btype != deflate_parse.STORED:
            marker = blocks[i + 1]
            assert marker.btype == deflate_parse.STORED and marker.nbytes == 0 and not marker.final
            i += 1
        i += 1
    return out


def select(cands, span, plain_len, header_len):
    """index_select (inflate_index_plan.h), restated"""
    pts = [(8 * header_len, 0, 0)]
    for bit, out_off in cands:
        if out_off < pts[-1][1] + span or out_off >= plain_len or bit <= pts[-1][0]:
            continue
        pts.append((bit, out_off, min(32768, out_off)))
    return pts


def span_bound_holds(pts, plain_len, span):
    ends = [p[1] for p in pts[1:]] + [plain_len]
    return all(e - p[1] < span + SLACK for p, e in zip(pts, ends))


# ---- reads --------------------------------------------------------------------------------------------------------------------
def read_check(torch, idx, src, plain, ranges, scratch=0):
    """`ranges` = [(uoff, len, alignment)].  Reads them into one arena, compares the WHOLE arena with the expected one (status 1,
    the clipped slice in place, 0xAB everywhere else) and returns the counters."""
    offs, at = [], 0
    for uoff, length, align in ranges:
        at = ((at + GUARD + 15) & ~15) + align
        offs.append(at)
        at += length
    arena = torch.full((at + GUARD + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    assert arena.data_ptr() % 16 == 0
    expect = np.full(arena.numel(), 0xAB, dtype=np.uint8)
    rc, out, counters = idx.read(src, [(u, n, arena.data_ptr() + o) for (u, n, _), o in zip(ranges, offs)], scratch_bytes=scratch)
    torch.cuda.synchronize()
    assert rc == 0
    for k, ((uoff, length, _), o) in enumerate(zip(ranges, offs)):
        clipped = max(0, min(length, len(plain) - uoff))
        assert out[k] == (1, clipped, None), (k, ranges[k], out[k])
        expect[o:o + clipped] = np.frombuffer(plain[uoff:uoff + clipped], dtype=np.uint8)
    got = arena.cpu().numpy()
    bad = np.nonzero(got != expect)[0]
    assert bad.size == 0, ("first differing arena byte", int(bad[0]), "of", bad.size)
    return counters
