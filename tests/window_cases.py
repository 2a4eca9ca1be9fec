"""Planted repeats for deflate at windowBits 9..14 (test infrastructure; pure numpy, seeded): the cells of matcher_cases.py with
the distance cap of a SMALLER window, cap(w) = (1 << w) - 262 = MAX_DIST(s) (deflate.h:410-415).  matcher_cases.MAX_DIST and
planted_dict are fixed at 32506, so the generators that need their own cap live here; the forms (far, near, dictionary), the
coverage measure and the packing are matcher_cases' own.

Per window w:
  position cells   m in (16, 300), D in (1, 7, cap - 1, cap), at in AT wherever at >= D: the rows batch (5120), the block
                   (61440) and the 128 KiB segment border (131072), one byte to either side of each.  At w 9 and 10 the cap is
                   below one 1024-position batch, at 11 it spans two.  D = cap at at = 131072 is the repeat whose source lies
                   exactly cap in front of a segment's first byte: the priming must have entered it.
  too-far cells    D in (cap + 1, 1 << w, 32506) at at = 40000: the only copy lies beyond the window, nothing may be found.
                   (m = 300 with D = cap + 1 < 300 is the near form: its copies lie at multiples of D, all too far.)
  dictionary cells a history of 300 and of 32768 bytes in front of the stream, R once in the history and once in the stream,
                   cap apart (found) and cap + 1 apart (too far).  R stands as far back in the history as the distance allows, so
                   behind a 32768-byte history the stream begins with R and most of the history lies beyond the window.

reader(w) is CPython's zlib as a reader that really has a 1 << w window: decompressobj(-w) fed with max_length = 97, so that
copies go through its window.  (A whole-buffer decode proves nothing: zlib then copies straight from the output buffer and
accepts a distance-600 stream at wbits 9.)"""
import functools
import zlib

import numpy as np

import matcher_cases as mc

WINDOWS = (9, 10, 11, 12, 13, 14)
LENGTHS = (16, 300)
AT = (5119, 5120, 5121, 61440, 131071, 131072, 131073)
TOO_FAR_AT = 40000
DICT_LENS = (300, 32768)
DICT_M = 16
CHUNK = 97



def cpython_misses(c, level):
    """The (cell, level) pairs at which CPython's zlib (1.2.11) itself does not meet the recall rule at its own window, found by
    test_window_cases_cpu.py, which holds it to every other pair: at w = 9, level 1, the 300-byte ranges at D = 7, 249 and 250
    (deflate_fast does not enter the strings of a long match, and behind its first 258-byte match it goes 7 or 42 bytes
    without one).  The oracle does not show that recall there, so the recall of these pairs is not asked of the device
    either; the cap is."""
    return c.w == 9 and level == 1 and c.m == 300 and c.sweep == "pos" and c.D in (7, 249, 250)


def cap(w):
    return (1 << w) - 262


def _cell(w, c):
    c.w = w
    c.too_far = c.D > cap(w)
    c.name = "w%d/%s" % (w, c.name)
    return c


def planted(w, m, D, at, tail=300):
    return _cell(w, mc.planted("pos" if D <= cap(w) else "far", m, D, at, tail, salt=w))


def planted_dict(w, m, dict_len, D, tail=300):
    """R in the history and again in the stream, D apart, as far back in the history as D allows"""
    src = max(dict_len - D, 0)
    off = D - (dict_len - src)
    assert m <= D and src + m <= dict_len and off >= 0
    rng = np.random.default_rng(mc._seed(w, m, dict_len, D, 7))
    r = mc.distinct_bytes(m, rng)
    history = bytes(src) + r + bytes(dict_len - src - m)
    return _cell(w, mc.Cell("dict", m, D, off, tail, bytes(off) + r + bytes(tail), history))


@functools.lru_cache(maxsize=None)
def cells(w):
    out = []
    for m in LENGTHS:
        for D in (1, 7, cap(w) - 1, cap(w)):
            out += [planted(w, m, D, at) for at in AT if at >= D]
        out += [planted(w, m, D, TOO_FAR_AT) for D in (cap(w) + 1, 1 << w, 32506)]
    for dict_len in DICT_LENS:
        out += [planted_dict(w, DICT_M, dict_len, D) for D in (cap(w), cap(w) + 1)]
    assert len({c.name for c in out}) == len(out)
    return out


def ranges(c):
    """the ranges of a cell that are judged on their own: the rows class ends every match at its segment's end"""
    b = mc.segment_border(c)
    return [(c.at, b), (b, c.at + c.m)] if b else [(c.at, c.at + c.m)]


def distance_ok(c, d):
    return d % c.D == 0 if c.near else d == c.D


def recall(c, parsed, allowance=3, split=True):
    """[(literal bytes, distances)] per judged range, and whether the rule of test_rows_recall holds: at most `allowance`
    literal bytes per range, every overlapping match at distance D (far form) or a multiple of D (near form).  split: the
    rows class's ranges (cut at the segment border); a compressor with one segment is judged on the whole range"""
    out, ok = [], True
    for lo, hi in (ranges(c) if split else [(c.at, c.at + c.m)]):
        cov = mc.coverage(parsed, lo, hi, len(c.history))
        out.append((cov.lits, sorted(cov.dists)))
        ok &= cov.lits <= allowance and all(distance_ok(c, d) for d in cov.dists)
        ok &= bool(cov.dists) or hi - lo < 4
    return out, ok


def limits(c, parsed):
    """None, or what is wrong: a distance above the cap, a copy from in front of history + stream, a too-far range that is
    not literals throughout"""
    cov = mc.coverage(parsed, 0, 0, len(c.history))
    if cov.max_dist > cap(c.w) or cov.min_reach < 0:
        return ("limit", cov.max_dist, cov.min_reach)
    if c.too_far:
        cov = mc.coverage(parsed, c.at, c.at + c.m, len(c.history))
        if cov.dists or cov.lits != c.m:
            return ("too far", cov.lits, sorted(cov.dists))
    return None


def reader(wbits, comp, zdict=None, chunk=CHUNK):
    """(plaintext, eof, unused_data) through zlib.decompressobj(wbits) in pieces of `chunk` output bytes; raises zlib.error as the
    reader does"""
    d = zlib.decompressobj(wbits, zdict) if zdict is not None else zlib.decompressobj(wbits)
    out, buf = [], bytes(comp)
    while not d.eof:
        piece = d.decompress(buf, chunk)
        buf = d.unconsumed_tail
        if not piece and not buf:
            break
        out.append(piece)
    return b"".join(out), d.eof, d.unused_data
