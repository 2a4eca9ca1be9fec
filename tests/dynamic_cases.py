"""Crafted dynamic-Huffman blocks (test infrastructure): ONE list of cases for every inflate decoder of the project -- the
host token decoder, the device stream kernel, part mode in both LDS layouts, the sub-start parse, the block-start finder.
Every case controls what an encoder never lets a test control: which symbol gets a code of which length (1..15 bits, on
either side of every root: literal 10, distance 9 for whole streams and 8 for parts), how the lengths are written (each
repeat code at its edges, HCLEN, the code-length code itself), and which of the sets inflate_table permits although they are
incomplete (inftrees.c:126-137).  The invalid cases are the header errors of inflate.c:808-917 and the code errors behind
them.  Built with tests/deflate_craft.py; expected bytes are replay()'s, expected errors the oracle's.

A case: name, kind (its header's kind -- the finder tests want every kind on its share of the blocks), emit(bits, final)
(writes its block(s) at any bit position), tokens, needs (bytes of history its copies reach back into), and, for the case
on its own behind HISTORY[-needs:], stream and plain (None: the oracle refuses it)."""
import functools

import numpy as np

import deflate_craft as craft
import inflate_util

HISTORY = bytes(np.random.default_rng(0xD1CE).integers(0, 256, size=32768, dtype=np.uint8))
EOB = 256


class Case:
    def __init__(self, name, kind, emit, tokens=(), needs=0, valid=True):
        self.name, self.kind, self.emit, self.tokens, self.needs = name, kind, emit, list(tokens), needs
        b = craft.Bits()
        emit(b, True)
        b.align()
        self.stream = bytes(b.out)
        self.plain = craft.replay(self.tokens, HISTORY[len(HISTORY) - needs:]) if valid else None

    @property
    def history(self):
        return HISTORY[len(HISTORY) - self.needs:]


_SETS = {}                                                # case name -> the code lengths it was built with


def _dyn(name, kind, tokens, lit_lens, dist_lens, needs=0, valid=True, **kw):
    _SETS[name] = (lit_lens, dist_lens)

    def emit(bits, final):
        craft.dynamic_block(bits, tokens, final, lit_lens, dist_lens, **kw)
    return Case(name, kind, emit, tokens, needs, valid)


def sparse_lens(n, lens):
    out = [0] * n
    for s, l in lens.items():
        out[s] = l
    return out


def order_lens(n, order):
    """order[i] gets i + 1 bits, the last two the same: the chain 1, 2, ..., L - 1, L, L"""
    return craft.chain_lens(n, order[:-2], order[-2:])


def _extras(table, sym):
    """the two ends of a symbol's extra bits: all 0 and all 1"""
    top = (1 << table[sym]) - 1
    return (0, top) if top else (0,)


def _pairs(lit_lens, dist_lens, rounds=1):
    """every length symbol of the set with every distance symbol of the set, extra bits all 0 / all 1 in turn, a literal of the
    set between two copies (each literal in turn)"""
    lits = [s for s in range(256) if lit_lens[s]]
    lens = [(s, e) for s in range(257, len(lit_lens)) if lit_lens[s] and s <= 285 for e in _extras(craft._LEN_EXTRA, s - 257)]
    dists = [(d, e) for d in range(min(len(dist_lens), 30)) if dist_lens[d] for e in _extras(craft._DIST_EXTRA, d)]
    toks, k = [("L", s) for s in lits], 0
    for r in range(rounds):
        for i, (ls, le) in enumerate(lens):
            for j, (ds, de) in enumerate(dists):
                # more than 200 pairs (the flat and chain sets of V1 with their 12+ length entries and 30+ distance entries):
                # one diagonal in len(lens) // 4 is kept, so every length entry still meets several distance entries and back
                if (i + j + r) % max(1, len(lens) // 4) and len(lens) * len(dists) > 200:
                    continue
                toks.append(("S", ls, le, ds, de))
                if lits:
                    toks.append(("L", lits[k % len(lits)]))
                    k += 1
    return toks


# V1: the literal/length chains.  position i of the order has i + 1 bits (the last two 15): past the 10th it is a long code
_A, _B = ord("a"), ord("b")
_LIT_ORDERS = {
    "depth-lit": [257, EOB, 264, 270, 285, _A, _B, 99, 100, 101, 102, 103, 104, 105, 106, 107],
    "depth-len": [_A, EOB, 258, _B, 99, 100, 101, 102, 103, 104, 257, 264, 270, 280, 284, 285],
    "depth-eob": [_A, _B, 257, 264, 99, 100, 101, 102, 103, 104, 270, 105, 285, 106, 107, EOB],
}
# ... and the distance chains: D1 has symbols 7 / 8 / 9 on 8 / 9 / 10 bits and 10..15 behind every root; D2 the far symbols 29..14
# the other way round; D3 the symbols with the most extra bits on 8, 9 and 10 bits
_DIST_ORDERS = {"d1": list(range(16)), "d2": list(range(29, 13, -1)), "d3": [0, 1, 2, 3, 4, 5, 6, 27, 28, 29, 20, 21, 22, 23, 24, 25]}


def _v1():
    out = []
    for kind, order in _LIT_ORDERS.items():
        lit = order_lens(286, order)
        for dn, dorder in _DIST_ORDERS.items():
            dist = order_lens(30, dorder)
            out.append(_dyn("%s/%s" % (kind, dn), kind, _pairs(lit, dist), lit, dist, needs=32768))
    lit = craft.flat_lens(286)
    for dn, dorder in _DIST_ORDERS.items():
        dist = order_lens(30, dorder)
        toks = [("L", 7 * i % 256) for i in range(40)] + _pairs(sparse_lens(286, {_A: 1, 257: 1, 263: 1, 285: 1}), dist)
        out.append(_dyn("depth-dist/%s" % dn, "depth-dist", toks, lit, dist, needs=32768))
    return out


def _v2():
    out = []
    lit, dist = craft.flat_lens(286), craft.flat_lens(30)
    lens = [(s, e) for s in range(257, 286) for e in _extras(craft._LEN_EXTRA, s - 257)]
    dists = [(d, e) for d in range(30) for e in _extras(craft._DIST_EXTRA, d)]

    def toks():
        t = []
        for i in range(len(dists)):
            t += [("S",) + lens[i % len(lens)] + dists[i], ("L", 65 + i % 26)]
        for i in range(len(dists)):
            t += [("S",) + lens[(7 * i + 1) % len(lens)] + dists[(11 * i) % len(dists)]]
        return t
    out.append(_dyn("syms-flat", "syms-flat", toks(), lit, dist, needs=32768))
    # V3: 284 with extra 31 is 258 bytes, as 285 is (inflate accepts both)
    v3 = [("L", 1), ("S", 284, 31, 0, 0), ("S", 285, 0, 0, 0), ("L", 2), ("S", 284, 30, 1, 0), ("S", 284, 31, 29, 8191),
          ("S", 285, 0, 29, 8191), ("S", 284, 31, 4, 1), ("L", 3)]
    out.append(_dyn("syms-284+31", "syms-flat", v3, lit, dist, needs=32768))
    # every length symbol and the end-of-block on 15 bits (12 in the third), the distance symbols on 15 bits in two halves
    deep = list(range(257, 286)) + [EOB, 120, 121]
    lit15 = craft.chain_lens(286, list(range(97, 107)), deep)
    lit12 = craft.chain_lens(286, list(range(97, 104)), deep)
    dist_a = craft.chain_lens(30, list(range(16, 27)), list(range(16)))
    dist_b = craft.chain_lens(30, list(range(11)), list(range(14, 30)))
    for name, ll, dl in (("syms-long/a", lit15, dist_a), ("syms-long/b", lit15, dist_b), ("syms-long/12", lit12, dist)):
        t = [x for x in toks() if x[0] == "L" or dl[x[3]]]
        out.append(_dyn(name, "syms-long", [("L", 97 + k % 7) if x[0] == "L" else x for k, x in enumerate(t)], ll, dl, needs=32768))
    return out


_SMALL = {_A: 1, _B: 2, 99: 3, EOB: 4, 257: 5, 258: 5}       # a small complete set; HLIT = 257 without the two length symbols
_SMALL257 = {_A: 1, _B: 2, 99: 3, EOB: 3}


def _text(n, syms=(_A, _B, 99)):
    return [("L", syms[(i * i + i // 3) % len(syms)]) for i in range(n)]


def _v4():
    small = sparse_lens(259, _SMALL)
    return [
        _dyn("dist-none", "dist-none", _text(40), sparse_lens(257, _SMALL257), [0]),
        _dyn("dist-one/0", "dist-one", _text(5) + [("M", 3, 1), ("L", _B), ("M", 4, 1)], small, [1]),
        _dyn("dist-one/4", "dist-one", _text(8) + [("M", 3, 5), ("L", _B), ("M", 4, 6)], small, [0, 0, 0, 0, 1]),
        _dyn("dist-two", "dist-two", _text(5) + [("M", 3, 1), ("M", 4, 2), ("L", 99), ("M", 3, 2)], small, [1, 1]),
        _dyn("dist-all", "dist-all", _text(5) + [("M", 3 + d % 2, craft._DIST_BASE[d]) for d in range(30)], small,
             craft.flat_lens(30), needs=32768),
    ]


def _v5():
    def empty(bits, final):                               # on its own: three empty blocks, then a fourth, the final one
        for k in range(4 if final else 1):
            craft.dynamic_block(bits, [], final and k == 3, sparse_lens(257, {EOB: 1}), [0])
    top = sparse_lens(286, {_A: 1, _B: 2, EOB: 3, 285: 4, 284: 4})
    return [
        Case("lit-empty", "lit-empty", empty),
        _dyn("lit-hlit257", "lit-hlit", _text(60), sparse_lens(257, _SMALL257), [0]),
        _dyn("lit-hlit286", "lit-hlit", _text(9, (_A, _B)) + [("M", 258, 2), ("S", 284, 31, 1, 0), ("L", _A)], top, [1, 1]),
        # 255 literals and the end-of-block on 8 bits, written one length after the other with the least HCLEN
        _dyn("lit-hclen5/plain", "lit-hclen5", [("L", i) for i in range(0, 255, 2)], [8] * 255 + [0, 8], [0],
             cl_lens=sparse_lens(19, {0: 1, 8: 1}), cl_syms=[8] * 255 + [0, 8, 0], hclen=5),
        _dyn("lit-hclen5/16", "lit-hclen5", [("L", i) for i in range(254, 0, -3)], [8] * 255 + [0, 8], [0],
             cl_lens=sparse_lens(19, {0: 2, 8: 1, 16: 2}), hclen=5),
    ]


# V6: one pair of sets written in many ways.  96 literals, the end-of-block and 15 length symbols on 6 / 7 bits, zeros in
# front, between and behind; the distance lengths begin with zeros too, so that one run of zeros spans the border
def _v6_sets():
    syms = list(range(32, 128)) + [EOB] + list(range(257, 272))
    lit = [0] * 276
    for s, l in zip(syms, craft.flat_lens(len(syms))):
        lit[s] = l
    return lit, [0, 0, 0, 0] + [3] * 8


def _v6():
    lit, dist = _v6_sets()
    toks = [("L", 32 + (5 * i) % 96) for i in range(30)] + [("M", 3 + i, craft._DIST_BASE[4 + i % 8]) for i in range(15)]
    seq = lit + dist
    out = [_dyn("hdr-rle/%s" % st, "hdr-rle", toks, lit, dist, cl_syms=craft.rle(seq, st, border=len(lit)))
           for st in ("plain", "greedy", "max", "cross")]
    # ... and "max" where a zero run is longer than 138 (156 zeros behind 'c', 97 in front of 'a'): 18 x 138, then 17 x 10
    wide = sparse_lens(257, _SMALL257)
    long_max = craft.rle(wide + [0], "max")
    assert (18, 138) in long_max and long_max.count((17, 10)) >= 9
    out.append(_dyn("hdr-rle/max-138", "hdr-rle", _text(40), wide, [0], cl_syms=long_max))
    # a 16 directly behind a run of zeros repeats the 0: the last three of every long zero run
    after = []
    for s in craft.rle(seq, "cross", border=len(lit)):
        if isinstance(s, tuple) and s[0] in (17, 18) and s[1] - 3 >= (11 if s[0] == 18 else 3):
            after += [(s[0], s[1] - 3), (16, 3)]
        else:
            after.append(s)
    assert sum(1 for a, b in zip(after, after[1:]) if isinstance(a, tuple) and a[0] == 18 and b == (16, 3)) >= 1
    assert sum(1 for a, b in zip(after, after[1:]) if isinstance(a, tuple) and a[0] == 17 and b == (16, 3)) >= 1
    out.append(_dyn("hdr-16/behind-zeros", "hdr-16", toks, lit, dist, cl_syms=after))
    # a 16 that repeats the last literal/length length into the distance lengths; it is also the header's last symbol
    lit4, dist4 = sparse_lens(259, {_A: 1, _B: 2, EOB: 3, 257: 4, 258: 4}), [4] * 16
    into = craft.rle(lit4 + dist4, "cross", border=259)
    assert into[-1] == (16, 5)
    t4 = _text(20, (_A, _B)) + [("M", 3 + d % 2, craft._DIST_BASE[d]) for d in range(9)]
    out.append(_dyn("hdr-16/into-dist", "hdr-16", t4, lit4, dist4, cl_syms=into))
    # a 17 / an 18 that ends exactly at HLIT + HDIST
    for name, dl in (("hdr-16/ends-17", [1, 1] + [0] * 5), ("hdr-16/ends-18", [1, 1] + [0] * 28)):
        syms = craft.rle(lit4 + dl, "greedy", border=259)
        assert syms[-1] in ((17, 5), (18, 28))
        out.append(_dyn(name, "hdr-16", _text(9, (_A, _B)) + [("M", 4, 2), ("M", 3, 1)], lit4, dl, cl_syms=syms))
    # the code-length code itself: members of 7 bits; two symbols of 1 bit
    used = craft.rle(seq, "greedy", border=len(lit))
    cl7 = sparse_lens(19, dict(zip([7, 6, 18, 3, 0, 16, 17, 5], [1, 2, 3, 4, 5, 6, 7, 7])))
    assert all(cl7[s[0] if isinstance(s, tuple) else s] for s in used)
    out.append(_dyn("hdr-cl/7bit", "hdr-cl", toks, lit, dist, cl_lens=cl7, cl_syms=used))
    two = sparse_lens(257, {_A: 1, EOB: 1})
    out.append(_dyn("hdr-cl/two-1bit", "hdr-cl", _text(30, (_A,)), two, [0], cl_lens=sparse_lens(19, {0: 1, 1: 1}),
                    cl_syms=two + [0]))
    return out


# V7: n literals of ONE bit shift everything behind them by n bits: a 15-bit distance code with 13 extra bits at every bit
# offset around stream byte 256 and 512 (the decode loop fetches 64 words at a time)
_V7_LIT = sparse_lens(258, {_A: 1, 257: 2, EOB: 3, _B: 3})
_V7_DIST = craft.chain_lens(30, list(range(14)), [28, 29])


def _v7():
    b = craft.Bits()
    craft.dynamic_block(b, [], True, _V7_LIT, _V7_DIST, eob=False)
    header = b.bit_length()
    out = []
    for byte in (256, 512):
        n0 = 8 * byte - header - 2 - 40                   # the code begins 40 bits in front of the byte ... 23 bits behind it
        for n in range(n0, n0 + 64):
            toks = [("L", _A)] * n + [("S", 257, 0, 28 + n % 2, (n * 2654435761 >> 7) & 0x1fff), ("L", _B), ("L", _A)]
            out.append(_dyn("refill/%d/%d" % (byte, n - n0), "refill", toks, _V7_LIT, _V7_DIST, needs=32768))
    return out


@functools.lru_cache(maxsize=None)
def valid_cases():
    cases = _v1() + _v2() + _v4() + _v5() + _v6() + _v7()
    assert len({c.name for c in cases}) == len(cases)
    return cases


def kinds():
    out = []
    for c in valid_cases():
        if c.kind not in out:
            out.append(c.kind)
    return out


# ---- invalid ----------------------------------------------------------------------------------------------------------------
def _bad(name, tokens, lit_lens, dist_lens, tail=(), **kw):
    """a block the oracle refuses; tail: (value, nbits) written behind the tokens instead of an end-of-block"""
    def emit(bits, final):
        craft.dynamic_block(bits, tokens, final, lit_lens, dist_lens, eob=not tail, **kw)
        for v, n in tail:
            bits.put(v, n)
    return Case(name, "invalid", emit, tokens, valid=False)


def _fixed_bad(name, tokens):
    def emit(bits, final):
        craft.fixed_block(bits, tokens, final)
    return Case(name, "invalid", emit, tokens, valid=False)


def _invalid_blocks():
    small, d2 = sparse_lens(259, _SMALL), [1, 1]
    seq = small + d2
    plain = craft.rle(seq, "plain")
    t = _text(6)
    flat = craft.flat_lens(286)
    cases = [
        _bad("hlit-30", t, craft.flat_lens(287), d2), _bad("hlit-31", t, craft.flat_lens(288), d2),
        _bad("hdist-30", t, flat, craft.flat_lens(31)), _bad("hdist-31", t, flat, craft.flat_lens(32)),
        _bad("cl-incomplete", t, small, d2, cl_lens=sparse_lens(19, {0: 1, 1: 2, 2: 3, 3: 4, 4: 5, 5: 5, 18: 6})),
        _bad("cl-over", t, small, d2, cl_lens=sparse_lens(19, {0: 1, 1: 2, 2: 2, 3: 3, 4: 3, 5: 3, 18: 3})),
        _bad("16-first", t, small, d2, cl_syms=[(16, 3)] + plain[3:]),
        _bad("16-overrun", t, small, d2, cl_syms=plain[:-2] + [(16, 3)]),
        _bad("17-overrun", t, small, d2, cl_syms=plain[:-2] + [(17, 3)]),
        _bad("18-overrun", t, small, d2, cl_syms=plain[:-10] + [(18, 11)]),
        _bad("no-eob", t, sparse_lens(259, {_A: 1, _B: 2, 99: 3, 257: 4, 258: 4}), d2, tail=[(0, 16)]),
        _bad("lit-over", t, sparse_lens(259, {_A: 1, _B: 2, 99: 3, EOB: 3, 257: 5}), d2),
        _bad("lit-incomplete", t, sparse_lens(259, {_A: 1, _B: 2, 99: 3, EOB: 4}), d2),
        _bad("lit-one-2bit", [], sparse_lens(257, {EOB: 2}), [0]),
        _bad("dist-over", t, small, [1, 1, 2]),
        _bad("dist-two-2bit", t, small, [2, 2]),
        _bad("dist-one-2bit", t, small, [2]),
        _bad("dist-unused-code", t + [("S", 257, 0, None, 0)], small, [1], tail=[(1, 1), (0, 15)]),
        _bad("dist-none-length", t + [("S", 257, 0, None, 0)], small, [0], tail=[(0, 16)]),
        _fixed_bad("fixed-286", t + [("S", 286, 0, None, 0)]), _fixed_bad("fixed-287", t + [("S", 287, 0, None, 0)]),
        _fixed_bad("fixed-dist-30", t + [("S", 257, 0, 30, 0)]), _fixed_bad("fixed-dist-31", t + [("S", 257, 0, 31, 0)]),
    ]
    # one byte too far back through a long distance code: 40 bytes of output, distance 41 = symbol 10 (11 bits in D1) extra 8
    lit = order_lens(286, _LIT_ORDERS["depth-lit"])
    far = [("L", _A)] * 40 + [("S", 257, 0, 10, 8)]
    cases.append(_bad("too-far-long-code", far, lit, order_lens(30, _DIST_ORDERS["d1"])))
    return cases


class Invalid:
    def __init__(self, name, stream, case=None):
        self.name, self.stream, self.case = name, stream, case
        self.expect = inflate_util.oracle_inflate(stream, cap=CAP)


CAP = 1024                                                # output room of the invalid cases and the truncation sweep


@functools.lru_cache(maxsize=None)
def invalid_cases():
    """every invalid block as a stream, and once more cut behind the byte its offending bits end in (the shortest prefix
    that the oracle refuses the same way)"""
    out = []
    for c in _invalid_blocks():
        whole = Invalid(c.name, c.stream + b"\x55" * 8, c)  # (bytes behind it: the decoder may not need them)
        assert whole.expect[0] == -3, (c.name, whole.expect[:2])
        out.append(whole)
        for cut in range(1, len(c.stream) + 1):
            if inflate_util.oracle_inflate(c.stream[:cut], cap=CAP)[:2] == whole.expect[:2]:
                out.append(Invalid(c.name + "/cut", c.stream[:cut]))
                break
        else:
            raise AssertionError(c.name)
    return out


def truncation_seeds():
    """six small headers of the kinds of V4 - V6 (no distance code, one, a 16 into the distance lengths, a 17 that ends the
    header, two code-length symbols of 1 bit, an empty block in front), each with some 40 bytes of codes behind it.  The
    end-of-block has ONE bit in all of them, so that most values of a last byte among the codes end the stream or break it:
    a sweep of headers alone would be "needs more input" nearly everywhere, which decides nothing."""
    e257 = sparse_lens(257, {EOB: 1, _A: 2, _B: 3, 99: 3})
    e258 = sparse_lens(258, {EOB: 1, _A: 2, _B: 3, 257: 3})
    e259 = sparse_lens(259, {EOB: 1, _A: 2, _B: 3, 257: 4, 258: 4})
    two = sparse_lens(257, {_A: 1, EOB: 1})
    text = _text(130)
    copies = _text(100, (_A, _B)) + [("M", 3, 1), ("L", _A), ("M", 3, 1)] + _text(20, (_A, _B))
    seeds = []
    for lit, dist, toks, kw in (
            (e257, [0], text, {}),
            (e258, [1], copies, {}),
            (e259, [4] * 16, copies + [("M", 4, 4)], dict(cl_syms=craft.rle(e259 + [4] * 16, "cross", border=259))),
            (e258, [1, 1, 0, 0, 0, 0, 0], copies + [("M", 3, 2)], {}),
            (two, [0], _text(170, (_A,)), dict(cl_lens=sparse_lens(19, {0: 1, 1: 1}), cl_syms=two + [0]))):
        b = craft.Bits()
        craft.dynamic_block(b, toks, True, lit, dist, **kw)
        b.align()
        seeds.append(bytes(b.out))
    b = craft.Bits()
    craft.dynamic_block(b, [], False, sparse_lens(257, {EOB: 1}), [0])
    craft.dynamic_block(b, text[:70], True, e257, [0], cl_syms=craft.rle(e257 + [0], "max"))
    b.align()
    seeds.append(bytes(b.out))
    assert all(len(s) <= 64 for s in seeds), [len(s) for s in seeds]
    return seeds


@functools.lru_cache(maxsize=None)
def truncation_sweep():
    """[(stream, oracle result)]: every seed cut at every length, the last byte with each of its 256 values"""
    out = []
    for s in truncation_seeds():
        for cut in range(1, len(s) + 1):
            for v in range(256):
                t = s[:cut - 1] + bytes([v])
                out.append((t, inflate_util.oracle_inflate(t, cap=CAP)))
    return out


# ---- one large stream of crafted blocks (part mode) ---------------------------------------------------------------------------
class Large:
    """comp: three stored blocks of noise, then crafted dynamic blocks, then a final stored block.  blocks: crafted blocks;
    share: kind -> its share of them; total: all blocks of the stream"""


def _stored_lookalike(s):
    """a byte 0 / 1 with LEN != 0 and NLEN = ~LEN behind it: the pattern find_headers_range (inflate_large.hip) takes for a
    stored block on a byte boundary, restated"""
    return any(s[i] & 0xfe == 0 and (s[i + 1] | s[i + 2]) and (s[i + 1] ^ s[i + 3]) == 0xff and (s[i + 2] ^ s[i + 4]) == 0xff
               for i in range(len(s) - 4))


def _noise(bits, rng, n, final=False):
    craft.stored_block(bits, bytes(rng.integers(0, 256, size=n, dtype=np.uint8)), final)


@functools.lru_cache(maxsize=None)
def large_stream(markers, min_bytes=128 << 10, big=0, bad=None, tiny=0, lead=True):
    """markers: every crafted block behind 00 00 ff ff (a part start by its pattern), else block follows block at whatever
    bit the last one ended on, and the kinds take turns so that each has its share.  big: so many blocks of at least 64 KiB
    (one of 160 KiB) of repeated V1 / V2 tokens among them.  bad: the name of an invalid case to put deep into the stream.
    tiny: at least so many crafted blocks (whole turns of the kinds), none with bytes that pass for a stored block's header: a
    dozen of the refill cases have them (zeros, then the ones of a 15-bit code), the finder takes each for a start, and such a
    part asks for a larger slot -- a hundred of them in one piece, and the pieces call leaves the stream to the sequential
    decoder (right bytes, but no parts to count).  lead=False: no noise in front -- the first blocks' copies
    reach into whatever precedes the stream (32 KiB of it)."""
    rng = np.random.default_rng(0xB10C + markers)
    cases = valid_cases()
    if not markers or tiny:                               # kinds in turn, each kind's cases in turn (sixteen of a long list)
        per = [[c for c in cases if c.kind == k and not (tiny and _stored_lookalike(c.stream))] for k in kinds()]
        # (were the finder's pattern to change, this filter would no longer keep what it takes for a start out -- the packed-layout
        # test's "no bytes for the sequential decoder" then fails, which is the check; that the filter finds any at all is this one)
        assert not tiny or sum(len(p) for p in per) < len(cases)
        per = [p[::len(p) // 16] if len(p) > 16 else p for p in per]
        turns = max(len(p) for p in per) * len(per)
        cases = [per[i % len(per)][(i // len(per)) % len(per[i % len(per)])] for i in range(turns)]
    b = craft.Bits()
    for _ in range(3 if lead else 0):
        _noise(b, rng, 40000)
    res = Large()
    res.blocks, res.total, count = 0, 3 if lead else 0, {}
    heavy = [c for c in valid_cases() if c.name in ("depth-lit/d1", "syms-long/a", "depth-len/d3", "syms-flat")]
    k, wrote_big, wrote_bad = 0, [], False                # (a long block takes the 7th place of every 40; the bad one comes in the second turn)
    while (tiny and res.blocks < tiny) or (not tiny and (b.bit_length() >> 3) < min_bytes + 120000) or k % len(cases):
        c = cases[k % len(cases)]
        k += 1
        if markers:
            craft.stored_block(b, b"", False)
            res.total += 1
        if big and k % 40 == 7 and k // 40 < big:
            h = heavy[(k // 40) % len(heavy)]
            reps = 5 * ((160 << 10) if k // 40 == 0 else (64 << 10)) // (4 * len(h.stream)) + 1      # (a quarter more: h.stream has the header in it)
            at = b.bit_length()
            craft.dynamic_block(b, h.tokens * reps, False, *_SETS[h.name])
            wrote_big.append((b.bit_length() - at) >> 3)
            count[h.kind] = count.get(h.kind, 0) + 1
            res.blocks += 1
            res.total += 1
            continue
        if bad and k == len(cases) + 5:
            bad_case = next(x.case for x in invalid_cases() if x.name == bad)
            bad_case.emit(b, False)
            wrote_bad = True
            break
        c.emit(b, False)
        count[c.kind] = count.get(c.kind, 0) + 1
        res.blocks += 1
        res.total += 1
    assert len(wrote_big) == big and all(n >= (64 << 10) for n in wrote_big) and (not big or max(wrote_big) >= (160 << 10)), wrote_big
    assert wrote_bad == bool(bad)
    for _ in range(2):
        _noise(b, rng, 40000)
    craft.stored_block(b, b"the end", True)
    res.total += 3
    res.comp = bytes(b.out)
    res.share = {kd: n / res.blocks for kd, n in count.items()}
    return res
