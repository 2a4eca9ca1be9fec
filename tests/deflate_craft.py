"""Raw deflate streams built token by token (test infrastructure): stored, fixed-Huffman and dynamic-Huffman blocks from
explicit ('L', byte) / ('M', length, distance) tokens, so that a test can put a copy of a chosen length at a chosen distance
at a chosen output position -- and, for dynamic blocks, from explicit code lengths: which symbol gets a code of which
length, how the lengths are written (the code-length code's own lengths, HCLEN, every repeat code and its run), whether the
end-of-block code is sent.  A raw token ('S', litlen symbol, length extra, distance symbol, distance extra) sends any
symbol with any extra-bit value (distance symbol None: the literal/length symbol alone).  Nothing here checks validity:
sets that inflate must refuse can be written as well as the permitted ones.  RFC 1951 3.2.5 - 3.2.7 (inftrees.c:38-49 and
inffixed_tbl.h hold the same tables; inflate.c:814-917 reads the dynamic header)."""

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
              8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):                   # LSB first (extra bits, header fields)
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def put_code(self, code, nbits):               # Huffman codes go in most significant bit first
        rev = int(format(code, "0%db" % nbits)[::-1], 2)
        self.put(rev, nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bit_length(self):
        return 8 * len(self.out) + self.n


def _fixed_litlen(sym):
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


def fixed_block(bits, tokens, final):
    bits.put(1 if final else 0, 1)
    bits.put(1, 2)
    for t in tokens:
        if t[0] == "L":
            bits.put_code(*_fixed_litlen(t[1]))
            continue
        if t[0] == "S":
            _put_raw(bits, t, _fixed_litlen, lambda d: (d, 5))
            continue
        _, length, dist = t
        k = max(i for i in range(29) if _LEN_BASE[i] <= length) if length < 258 else 28
        bits.put_code(*_fixed_litlen(257 + k))
        bits.put(length - _LEN_BASE[k], _LEN_EXTRA[k])
        d = max(i for i in range(30) if _DIST_BASE[i] <= dist)
        bits.put_code(d, 5)
        bits.put(dist - _DIST_BASE[d], _DIST_EXTRA[d])
    bits.put_code(*_fixed_litlen(256))


def stored_block(bits, data, final):
    assert len(data) <= 65535
    bits.put(1 if final else 0, 1)
    bits.put(0, 2)
    bits.align()
    bits.put(len(data), 16)
    bits.put(len(data) ^ 0xFFFF, 16)
    bits.out += data                               # aligned here


def replay(tokens, history=b""):
    """the bytes the tokens produce (history = what precedes the output)"""
    buf = bytearray(history)
    for t in tokens:
        if t[0] == "L":
            buf.append(t[1])
        else:
            if t[0] == "S":
                if t[1] < 256:
                    buf.append(t[1])
                    continue
                length, dist = _LEN_BASE[t[1] - 257] + t[2], _DIST_BASE[t[3]] + t[4]
            else:
                _, length, dist = t
            assert dist <= len(buf)
            for _ in range(length):
                buf.append(buf[-dist])
    return bytes(buf[len(history):])


def _put_raw(bits, t, litlen_code, dist_code):
    """('S', litlen symbol, length extra, distance symbol, distance extra): no symbol or value is refused"""
    _, sym, len_extra, dsym, dist_extra = t
    bits.put_code(*litlen_code(sym))
    if sym <= 256:
        return
    bits.put(len_extra, _LEN_EXTRA[sym - 257] if sym - 257 < 29 else 0)
    if dsym is None:
        return
    bits.put_code(*dist_code(dsym))
    bits.put(dist_extra, _DIST_EXTRA[dsym] if dsym < 30 else 0)


def match_symbols(length, dist):
    """('M', length, distance) as the raw token's fields: (litlen symbol, length extra, distance symbol, distance extra)"""
    k = max(i for i in range(29) if _LEN_BASE[i] <= length) if length < 258 else 28
    d = max(i for i in range(30) if _DIST_BASE[i] <= dist)
    return 257 + k, length - _LEN_BASE[k], d, dist - _DIST_BASE[d]


# ---- dynamic blocks (RFC 1951 3.2.7) --------------------------------------------------------------------------------------
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canonical_codes(lens):
    """symbol -> (code, nbits) of the canonical Huffman code with these lengths (RFC 1951 3.2.2); symbols of length 0 have
    none.  An over-subscribed set gets codes cut to their length: no decoder reaches them."""
    count = [0] * (max(lens, default=0) + 2)
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * len(count)
    for n in range(1, len(count)):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    out = {}
    for sym, n in enumerate(lens):
        if n:
            out[sym] = (nxt[n] & ((1 << n) - 1), n)
            nxt[n] += 1
    return out


def flat_lens(n):
    """n symbols, complete, every code one of two neighbouring lengths (the first 2^b - n symbols one bit shorter)"""
    b = max(1, (n - 1).bit_length())
    short = (1 << b) - n
    return [b - 1] * short + [b] * (n - short)


def chain_lens(n, short, deep):
    """a set of n lengths in which short[i] has i + 1 bits and the symbols of `deep` (a power of two of them) share what is
    left: complete.  Two deep symbols behind L - 1 short ones are the chain 1, 2, ..., L - 1, L, L."""
    m = len(deep).bit_length() - 1
    assert len(deep) == 1 << m and len(short) + m <= 15 and not set(short) & set(deep)
    lens = [0] * n
    for i, s in enumerate(short):
        lens[s] = i + 1
    for s in deep:
        lens[s] = len(short) + m
    return lens


def rle(seq, style, border=None):
    """the code lengths `seq` as code-length symbols: ints 0..15, or (16 | 17 | 18, run).  Styles: "plain" no repeats;
    "greedy" as an encoder writes them (longest run first, never across `border`, the end of the literal/length lengths);
    "max" runs of exactly 138 / 10 / 6 wherever they fit, what is left greedy; "cross" greedy over the whole sequence,
    and a run must span `border`."""
    if style == "plain":
        return list(seq)
    if style in ("greedy", "max") and border is not None:
        return rle(seq[:border], style) + rle(seq[border:], style)
    out, i, crossed = [], 0, False
    while i < len(seq):
        v, j = seq[i], i
        while j < len(seq) and seq[j] == v:
            j += 1
        run, start = j - i, i
        if v:                                       # the length itself, then 16s
            out.append(v)
            run -= 1
            i += 1
        while run >= 3:
            if v:
                step = 6 if run >= 6 else run
                sym = 16
            elif style == "max" and run < 138 and run >= 10:
                step, sym = 10, 17
            else:
                step = min(run, 138)
                sym = 18 if step >= 11 else 17
            out.append((sym, step))
            crossed |= border is not None and i < border < i + step
            i += step
            run -= step
        out += [v] * run
        i += run
        assert i == j and start <= i
    assert style != "cross" or crossed, "no run spans the border"
    return out


_CL_EXTRA = {16: (2, 3), 17: (3, 3), 18: (7, 11)}


def dynamic_block(bits, tokens, final, lit_lens, dist_lens, *, cl_lens=None, cl_syms=None, hclen=None, eob=True):
    """one dynamic block.  lit_lens / dist_lens: the code lengths, their sizes are HLIT + 257 / HDIST + 1 (any size is
    written: the fields are 5 bits); cl_syms: the code-length symbols that send them (default rle(..., "greedy"));
    cl_lens: the 19 lengths of the code-length code (default: complete, all 19 have codes); hclen: how many of them are sent
    (default: up to the last one that is not 0); eob=False: no end-of-block code, the caller goes on writing bits."""
    if cl_syms is None:
        cl_syms = rle(list(lit_lens) + list(dist_lens), "greedy", border=len(lit_lens))
    if cl_lens is None:
        cl_lens = flat_lens(19)
    if hclen is None:
        hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
    bits.put(1 if final else 0, 1)
    bits.put(2, 2)
    bits.put((len(lit_lens) - 257) & 31, 5)
    bits.put((len(dist_lens) - 1) & 31, 5)
    bits.put((hclen - 4) & 15, 4)
    for k in range(hclen):
        bits.put(cl_lens[CL_ORDER[k]], 3)
    cl = canonical_codes(cl_lens)
    for s in cl_syms:
        if isinstance(s, tuple):
            bits.put_code(*cl[s[0]])
            nbits, base = _CL_EXTRA[s[0]]
            bits.put(s[1] - base, nbits)
        else:
            bits.put_code(*cl[s])
    lit, dist = canonical_codes(lit_lens), canonical_codes(dist_lens)
    for t in tokens:
        if t[0] == "L":
            bits.put_code(*lit[t[1]])
            continue
        _put_raw(bits, t if t[0] == "S" else ("S",) + match_symbols(t[1], t[2]), lit.__getitem__, dist.__getitem__)
    if eob:
        bits.put_code(*lit[256])
