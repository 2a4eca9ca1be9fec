"""The dry parse behind ZNG_ROCM_INFLATE_SUBBLOCK (subblock_sync_kernel, inflate_dev.hip), restated in Python for fixed
codes: from a guessed bit inside a fixed-Huffman block, parse K symbols and report the bit where the next one starts.
A guess that starts off the symbol grid falls onto it within a few symbols, so that bit is a true symbol boundary of the
block; a code the fixed tables do not have, or an end of block too early, restarts the parse one bit further on.  This
pins K = 128 against the symbol boundaries of a Python-side walk of the same stream (no GPU): with K = 64, 98.9 % of
guesses land on a boundary; with 128, 99.9 %."""
import os
import re
import zlib

import numpy as np

import synth

K = 128                                                   # kSyncSymbols: the rate below was checked with these
RESTARTS = 32                                             # kSyncRestarts
KERNEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zlib-ng_amd", "csrc", "inflate_dev.hip")


def test_kernel_uses_the_pinned_constants():
    """the sync kernel's K and restart count are the ones this restatement checks"""
    src = open(KERNEL).read()
    m = re.search(r"constexpr int kSyncSymbols = (\d+), kSyncRestarts = (\d+);", src)
    assert m, "kSyncSymbols / kSyncRestarts not found in inflate_dev.hip"
    assert (int(m.group(1)), int(m.group(2))) == (K, RESTARTS)


def _fixed_tables():
    """literal/length: 9 stream bits (first bit in bit 0) -> (symbol, code length); distance: 5 bits -> symbol"""
    lit = [None] * 512
    for sym in range(288):
        if sym < 144:
            code, n = 0x30 + sym, 8
        elif sym < 256:
            code, n = 0x190 + sym - 144, 9
        elif sym < 280:
            code, n = sym - 256, 7
        else:
            code, n = 0xC0 + sym - 280, 8
        rev = int(format(code, "0%db" % n)[::-1], 2)      # deflate sends Huffman codes first bit first
        for hi in range(1 << (9 - n)):
            lit[rev | (hi << n)] = (sym, n)
    dist = [int(format(c, "05b")[::-1], 2) for c in range(32)]
    return lit, dist


LIT, DIST = _fixed_tables()


def _len_extra(sym):
    k = sym - 257
    return 0 if k < 8 or k == 28 else (k - 4) >> 2


def _dist_extra(d):
    return 0 if d < 4 else (d - 2) >> 1


class Bits:
    def __init__(self, data):
        b = np.unpackbits(np.frombuffer(data + bytes(16), dtype=np.uint8), bitorder="little").astype(np.uint32)
        self.n = 8 * len(data)
        w = np.zeros(b.size - 32, dtype=np.uint32)
        for i in range(32):
            w |= b[i:i + w.size] << np.uint32(i)
        self.w = w                                        # w[p]: the 32 bits from bit p on

    def get(self, p, n):
        return int(self.w[p]) & ((1 << n) - 1)


def walk(bits):
    """every block of the stream: (type, first symbol bit, end bit) and the set of symbol boundaries of fixed blocks"""
    p, blocks, bounds = 0, [], set()
    while True:
        final, typ = bits.get(p, 1), bits.get(p + 1, 2)
        p += 3
        if typ == 0:
            p = (p + 7) & ~7
            ln = bits.get(p, 16)
            p += 32 + 8 * ln
            blocks.append((0, p, p))
        elif typ == 1:
            first = p
            while True:
                bounds.add(p)
                sym, n = LIT[bits.get(p, 9)]
                p += n
                if sym == 256:
                    break
                if sym > 256:
                    p += _len_extra(sym)
                    d = DIST[bits.get(p, 5)]
                    p += 5 + _dist_extra(d)
            blocks.append((1, first, p))
        else:
            raise AssertionError("a Z_FIXED stream holds fixed and stored blocks only")
        if final:
            return blocks, bounds


def _parse(bits, g):
    p = g
    for k in range(K):
        sym, n = LIT[bits.get(p, 9)]
        if sym == 256:
            return p if k >= K // 2 else None
        if sym > 285:
            return None
        p += n
        if sym > 256:
            p += _len_extra(sym)
            d = DIST[bits.get(p, 5)]
            if d > 29:
                return None
            p += 5 + _dist_extra(d)
    return p


def dry_parse(bits, g):
    """the sync kernel's dry parse with fixed codes: the boundary after K symbols, or the one in front of an end-of-block
    code met after K / 2; a code the fixed tables do not have or an earlier end of block starts it again one bit on"""
    for r in range(RESTARTS + 1):
        got = _parse(bits, g + r)
        if got is not None:
            return got
    return None


def test_fixed_code_guesses_land_on_symbol_boundaries():
    plain = synth.silesia_like(1 << 20, seed=0x5C).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
    comp = c.compress(plain) + c.flush()
    bits = Bits(comp)
    blocks, bounds = walk(bits)
    fixed = [(a, b) for t, a, b in blocks if t == 1 and b - a > 4096]
    assert fixed and sum(b - a for a, b in fixed) > 4 * bits.n // 5
    rng = np.random.default_rng(0x5B)
    lens = np.array([b - a for a, b in fixed], dtype=np.float64)
    picks = rng.choice(len(fixed), size=2000, p=lens / lens.sum())
    good = none = 0
    for i in picks:
        a, b = fixed[i]
        g = int(rng.integers(a, b - 2048))
        got = dry_parse(bits, g)
        if got is None:
            none += 1
        elif got in bounds:
            good += 1
    assert good >= 0.99 * len(picks), (good, none, len(picks))
