"""An independent DEFLATE block parser (test infrastructure): a plain-Python bit reader that takes a raw deflate stream
apart block by block -- where each block starts, where its header ends, where it ends; for a dynamic block HLIT, HDIST,
HCLEN, the 19 lengths of the code-length code, the code-length symbols as they were sent (16 / 17 / 18 with their runs) and
the literal/length and distance lengths they spell; the tokens, the two histograms they make (end-of-block included) and the
bytes the block covers.  tests/deflate_craft.py only writes; this only reads, and shares nothing with it: the tables below
are RFC 1951's (3.2.5 - 3.2.7).

Every code set is checked on its own (Kraft sum): an over-subscribed set is always an error, an incomplete one is an error
when strict (the default) -- but for what RFC 1951 3.2.7 allows the distance code: one code of one bit, or none at all."""
import numpy as np

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
             6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
STORED, STATIC, DYNAMIC = 0, 1, 2
STATIC_LIT_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8           # 288 codes; 286 and 287 never occur in data
STATIC_DIST_LENS = [5] * 32


class ParseError(ValueError):
    pass


def kraft(lens):
    """(sum of 2^(15 - len) over the codes, 2^15): equal when the set is complete"""
    return sum(1 << (15 - n) for n in lens if n), 1 << 15


def code_state(lens):
    """'complete', 'over', 'incomplete', 'one' (a single code of one bit) or 'none' (no code at all)"""
    used = [n for n in lens if n]
    if not used:
        return "none"
    if used == [1]:
        return "one"
    have, full = kraft(used)
    return "complete" if have == full else ("over" if have > full else "incomplete")


def _table(lens):
    """peek table of the canonical code (RFC 1951 3.2.2): index = the next maxlen bits of the stream (first bit lowest),
    entry = symbol << 4 | length, -1 where no code begins"""
    maxlen = max(lens)
    if maxlen == 0:
        return [-1], 0
    count = [0] * (maxlen + 2)
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * (maxlen + 2)
    for n in range(1, maxlen + 1):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    tab = [-1] * (1 << maxlen)
    for sym, n in enumerate(lens):
        if not n:
            continue
        c = nxt[n]
        nxt[n] += 1
        if c >> n:
            raise ParseError("over-subscribed code set")
        rev = int(format(c, "0%db" % n)[::-1], 2)
        e = sym << 4 | n
        for i in range(rev, 1 << maxlen, 1 << n):
            tab[i] = e
    return tab, (1 << maxlen) - 1


class Block:
    """final, btype; start / header_end / end: bit offsets (a stored block's header ends behind NLEN);
    dynamic: hlit, hdist, hclen, cl_lens[19], cl_syms (ints 0..15, (16 | 17 | 18, run)), lit_lens[286], dist_lens[30];
    lit_syms: every literal/length symbol in order, end-of-block included (empty for a stored block);
    matches: (index into lit_syms, length, distance, distance symbol);  out_start, out_end: the bytes it covers."""

    def __init__(self):
        self.hlit = self.hdist = self.hclen = None
        self.cl_lens = self.cl_syms = self.lit_lens = self.dist_lens = None
        self.lit_syms, self.matches = [], []
        self.states = {}

    @property
    def header_bits(self):
        return self.header_end - self.start

    @property
    def nbytes(self):
        return self.out_end - self.out_start

    @property
    def lit_hist(self):
        return np.bincount(np.asarray(self.lit_syms, dtype=np.int64), minlength=286).tolist()

    @property
    def dist_hist(self):
        return np.bincount(np.asarray([m[3] for m in self.matches], dtype=np.int64), minlength=30).tolist()

    @property
    def cl_hist(self):
        h = [0] * 19
        for s in self.cl_syms or ():
            h[s[0] if isinstance(s, tuple) else s] += 1
        return h

    @property
    def tokens(self):
        """('L', byte) | ('M', length, distance), the form tests/deflate_craft.py writes"""
        out, at = [], {m[0]: m for m in self.matches}
        for i, s in enumerate(self.lit_syms):
            if s < 256:
                out.append(("L", s))
            elif s > 256:
                out.append(("M", at[i][1], at[i][2]))
        return out


class Parsed:
    def __init__(self, blocks, data, end_bit):
        self.blocks, self.data, self.end_bit = blocks, data, end_bit

    def bytes_of(self, b):
        return self.data[b.out_start:b.out_end]


def _check(state, what, strict, allow_one):
    if state == "over":
        raise ParseError("%s code set is over-subscribed" % what)
    if strict and (state == "incomplete" or (state in ("one", "none") and not allow_one)):
        raise ParseError("%s code set is incomplete (%s)" % (what, state))


def parse(stream, history=b"", strict=True):
    """Parsed(blocks, data, end_bit): every block up to and including the final one; data = the plaintext (without the
    history the first copies may reach back into); end_bit = the bit behind the final block."""
    src = bytes(stream)
    nbit_total = 8 * len(src)
    hist_len = len(history)
    out = bytearray(history)
    pos, acc, nb = 0, 0, 0                                 # next byte to load, bit accumulator, bits in it

    def need(n):
        nonlocal pos, acc, nb
        while nb < n:
            acc |= int.from_bytes(src[pos:pos + 8], "little") << nb
            pos += 8
            nb += 64

    def take(n):
        nonlocal acc, nb
        need(n)
        v = acc & ((1 << n) - 1)
        acc >>= n
        nb -= n
        return v

    def offset():
        return 8 * pos - nb

    blocks = []
    while True:
        b = Block()
        b.start = offset()
        b.final = take(1)
        b.btype = take(2)
        b.out_start = len(out) - hist_len
        if b.btype == 3:
            raise ParseError("block type 3")
        if b.btype == STORED:
            take((-offset()) % 8)
            ln, nln = take(16), take(16)
            if ln ^ nln != 0xffff:
                raise ParseError("stored block: NLEN is not ~LEN")
            b.header_end = offset()
            at = b.header_end >> 3
            if at + ln > len(src):
                raise ParseError("stored block runs past the end")
            out += src[at:at + ln]
            pos, acc, nb = at + ln, 0, 0
        else:
            if b.btype == DYNAMIC:
                b.hlit, b.hdist, b.hclen = take(5) + 257, take(5) + 1, take(4) + 4
                if b.hlit > 286 or b.hdist > 30:
                    raise ParseError("HLIT %d / HDIST %d" % (b.hlit, b.hdist))
                b.cl_lens = [0] * 19
                for k in range(b.hclen):
                    b.cl_lens[CL_ORDER[k]] = take(3)
                b.states["cl"] = code_state(b.cl_lens)
                _check(b.states["cl"], "code-length", strict, False)
                tab, mask = _table(b.cl_lens)
                lens, syms = [], []
                while len(lens) < b.hlit + b.hdist:
                    need(16)
                    e = tab[acc & mask]
                    if e < 0:
                        raise ParseError("no such code-length code")
                    acc >>= e & 15
                    nb -= e & 15
                    s = e >> 4
                    if s < 16:
                        lens.append(s)
                        syms.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise ParseError("repeat without a length before it")
                        run, v = 3 + take(2), lens[-1]
                    elif s == 17:
                        run, v = 3 + take(3), 0
                    else:
                        run, v = 11 + take(7), 0
                    lens += [v] * run
                    syms.append((s, run))
                if len(lens) != b.hlit + b.hdist:
                    raise ParseError("a run passes HLIT + HDIST")
                b.cl_syms = syms
                b.lit_lens = lens[:b.hlit] + [0] * (286 - b.hlit)
                b.dist_lens = lens[b.hlit:] + [0] * (30 - b.hdist)
                if not b.lit_lens[256]:
                    raise ParseError("no end-of-block code")
                lit_lens, dist_lens = b.lit_lens, b.dist_lens
            else:
                lit_lens, dist_lens = STATIC_LIT_LENS, STATIC_DIST_LENS
            b.header_end = offset()
            b.states["lit"], b.states["dist"] = code_state(lit_lens), code_state(dist_lens)
            _check(b.states["lit"], "literal/length", strict, False)
            _check(b.states["dist"], "distance", strict, True)
            ltab, lmask = _table(lit_lens)
            dtab, dmask = _table(dist_lens)
            lit_syms, matches = b.lit_syms, b.matches
            put_sym, put_byte = lit_syms.append, out.append
            while True:
                if nb < 48:
                    acc |= int.from_bytes(src[pos:pos + 8], "little") << nb
                    pos += 8
                    nb += 64
                e = ltab[acc & lmask]
                n = e & 15
                acc >>= n
                nb -= n
                s = e >> 4
                put_sym(s)
                if s < 256:
                    if e < 0:
                        raise ParseError("no such literal/length code")
                    put_byte(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise ParseError("literal/length symbol %d" % s)
                k = LEN_EXTRA[s - 257]
                length = LEN_BASE[s - 257] + (acc & ((1 << k) - 1))
                acc >>= k
                nb -= k
                e = dtab[acc & dmask]
                if e < 0:
                    raise ParseError("no such distance code")
                n = e & 15
                acc >>= n
                nb -= n
                d = e >> 4
                if d > 29:
                    raise ParseError("distance symbol %d" % d)
                k = DIST_EXTRA[d]
                dist = DIST_BASE[d] + (acc & ((1 << k) - 1))
                acc >>= k
                nb -= k
                if dist > len(out):
                    raise ParseError("distance %d reaches in front of the data" % dist)
                matches.append((len(lit_syms) - 1, length, dist, d))
                if dist >= length:
                    out += out[len(out) - dist:len(out) - dist + length]
                else:
                    for _ in range(length):
                        put_byte(out[-dist])
        b.end = offset()
        if b.end > nbit_total:
            raise ParseError("the stream ends inside a block")
        b.out_end = len(out) - hist_len
        blocks.append(b)
        if b.final:
            break
    return Parsed(blocks, bytes(out[hist_len:]), blocks[-1].end)


def data_blocks(p):
    """the blocks that carry data (or the one block of an empty input), without the design's additions: the empty stored
    block that byte-aligns every non-stored block, and the final empty static block"""
    blocks = p.blocks
    assert blocks[-1].final and blocks[-1].btype == STATIC and blocks[-1].nbytes == 0 and blocks[-1].end - blocks[-1].start == 10
    out, k = [], 0
    while k < len(blocks) - 1:
        b = blocks[k]
        assert b.start % 8 == 0, "every data block starts on a byte"
        out.append(b)
        k += 1
        if b.btype != STORED:
            m = blocks[k]
            assert m.btype == STORED and m.nbytes == 0 and not m.final, "the byte-aligning empty stored block"
            k += 1
    return out
