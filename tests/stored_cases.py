"""Crafted stored blocks (test infrastructure): ONE list of cases for every inflate decoder of the project -- the host token
decoder, the device stream kernel with its dictionary, span and part forms, and the sizing kernels.  An encoder writes a stored
block at bit 0 behind a zero pad with 65535 bytes in it; these stand on the edges of the code that reads one (RFC 1951 3.2.4,
inflate.c:759-800):
  the payload copy -- pieces of 1024 (RING / 4) bytes, 16 bytes a lane, a last lane that goes byte by byte, the ring's wrap;
  the flush -- due every RING / 2 bytes inside the piece loop, so that up to RING / 2 - 1 + 1024 bytes are unflushed when the
      block ends and the next block's first copy wants the newest bytes, a source beyond RING - 258 = 3838, or 258 bytes over
      the oldest ring slots;
  the bit buffer -- the header at each of the 8 bit offsets, pad bits that are not zero, LEN / NLEN across the border of the
      fetcher's 256-byte window, counted from the stream's start and from the seek behind a stored block;
  the waiting literals -- 63, 64 and 65 of them in front of the block;
  the ends -- NLEN that is not ~LEN, input that ends anywhere behind the header, room that ends anywhere in the payload.
Built with tests/deflate_craft.py; expected bytes are replay()'s and the payloads themselves, expected errors the oracle's.

A case: family, name, stream, plain (for `cuts`: what the complete blocks and the payload bytes present make), history (bytes in
front of the output), stored (one record per stored block: start_bit, hdr_byte -- the byte that holds that bit --, in_at /
out_at -- where the payload lies in stream / plain --, length, pad), meta (what the family varies)."""
import functools

import numpy as np

import deflate_craft as craft

LENS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 511, 512, 513, 1007, 1008, 1009, 1023, 1024, 1025, 1039, 1040, 1041, 2047,
        2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 65534, 65535)
FRONT = (0, 1, 63, 64, 65)                                   # literals in front (service() dumps up to 64 waiting ones)
PADS = ("zeros", "ones", "alt")
BIT_LENS = (0, 1, 17, 1025)
WINDOW_AT = tuple(range(250, 263)) + tuple(range(506, 519))  # the first byte of LEN, counted from the last seek
AFTER_LENS = (1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 3583, 3838, 4096, 65535)
AFTER_FRONT = (0, 300)
CUT_LENS = (0, 1, 17, 1025, 3073)
PAYLOAD_CUTS = (1, 15, 16, 17, 1023, 1024, 1025)             # ... and L - 1, for a payload of more than 64 bytes
HISTORY = bytes(np.random.default_rng(0x5701).integers(0, 256, size=32768, dtype=np.uint8))
_NOISE = np.random.default_rng(0x570BED).integers(0, 256, size=(1 << 20) + 65535, dtype=np.uint8).tobytes()


def after_distances(L, Q):
    """the distances of the `after` family behind Q literals and L stored bytes (none beyond what has been produced)"""
    want = (1, 2, 15, 16, 17, L, L + Q, 3837, 3838, 3839, 3840, 4095, 4096, 4097, min(32768, L + Q))
    return sorted({d for d in want if 1 <= d <= min(32768, L + Q)})


def stored_block(bits, data, final, pad="zeros", nlen=None):
    """a stored block with chosen pad bits (RFC 1951 ignores them; inflate.c:761 drops them) and any NLEN"""
    assert len(data) <= 65535
    bits.put(1 if final else 0, 1)
    bits.put(0, 2)
    k = (8 - bits.n) % 8
    bits.put({"zeros": 0, "ones": 0xff, "alt": 0x55}[pad] & ((1 << k) - 1), k)
    assert bits.n == 0
    bits.put(len(data), 16)
    bits.put(len(data) ^ 0xffff if nlen is None else nlen, 16)
    bits.out += data


class Stored:
    def __init__(self, start_bit, in_at, out_at, length, pad):
        self.start_bit, self.hdr_byte, self.in_at, self.out_at, self.length, self.pad = start_bit, start_bit >> 3, in_at, out_at, length, pad


class Case:
    def __init__(self, family, name, stream, plain, history=b"", stored=(), **meta):
        self.family, self.name, self.stream, self.plain, self.history = family, name, bytes(stream), bytes(plain), history
        self.stored, self.meta = list(stored), meta


class _Build:
    """a stream in the making: the bits, the plaintext so far, a record per stored block"""

    def __init__(self, history=b""):
        self.bits, self.plain, self.history, self.stored, self.at = craft.Bits(), bytearray(), history, [], 0

    def noise(self, n):
        """n bytes of seeded noise, another stretch of it at every call"""
        self.at = (self.at + 65537) % (1 << 20)
        return _NOISE[self.at:self.at + n]

    def literals(self, n, nine=0):
        """n literal tokens, the first `nine` of them with 9-bit codes (bytes of 144 and above), the others with 8-bit codes"""
        raw = self.noise(n)
        assert nine <= n
        return [("L", 144 + raw[i] % 112 if i < nine else raw[i] % 144) for i in range(n)]

    def fixed(self, tokens, final):
        craft.fixed_block(self.bits, tokens, final)
        if any(t[0] != "L" for t in tokens):
            tail = (self.history + bytes(self.plain))[-32768:] if len(self.plain) < 32768 else bytes(self.plain[-32768:])
            self.plain += craft.replay(tokens, tail)
        else:
            self.plain += bytes(t[1] for t in tokens)

    def store(self, data, final, pad="zeros", nlen=None):
        start = self.bits.bit_length()
        stored_block(self.bits, data, final, pad, nlen)
        self.stored.append(Stored(start, len(self.bits.out) - len(data), len(self.plain), len(data), pad))
        self.plain += data

    def case(self, family, name, **meta):
        self.bits.align()
        return Case(family, name, self.bits.out, self.plain, self.history, self.stored, **meta)


def _nine_count(tokens):
    return sum(1 for t in tokens if t[1] >= 144)


# ---- len: one stored block of every length, behind P literals, final or not ------------------------------------------------
def _len_case(L, P, final):
    b = _Build()
    if P:
        b.fixed(b.literals(P, nine=P // 3), False)
    b.store(b.noise(L), final, PADS[(L + P) % 3])
    if not final:
        b.fixed(b.literals(3), True)
    return b.case("len", "len/%d/%d/%s" % (L, P, "final" if final else "more"), L=L, P=P, final=final)


def _len():
    return [_len_case(L, P, final) for L in LENS for P in FRONT for final in (True, False)]


# ---- bit: the header at every bit offset, every pad -------------------------------------------------------------------------
def _bit():
    out = []
    for off in range(8):
        for pad in PADS:
            for L in BIT_LENS:
                # a fixed block of a 8-bit and b 9-bit literals takes 3 + 8 a + 9 b + 7 bits: it ends on bit (2 + b) mod 8
                b = _Build()
                nine = (off - 2) % 8
                toks = b.literals(3 + nine, nine=nine)
                assert _nine_count(toks) == nine
                b.fixed(toks, False)
                b.store(b.noise(L), True, pad)
                assert b.stored[0].start_bit % 8 == off
                out.append(b.case("bit", "bit/%d/%s/%d" % (off, pad, L), L=L, P=len(toks), off=off, pad=pad))
    return out


# ---- window: LEN / NLEN at the border of the fetcher's 256-byte window --------------------------------------------------------
def _window():
    out = []
    for base in ("start", "stored7"):
        for at in WINDOW_AT:
            b = _Build()
            seek = 0
            if base == "stored7":
                b.store(b.noise(7), False)
                seek = len(b.bits.out)
                assert seek == 12
            b.fixed(b.literals(at - 2), False)              # 10 + 8 (at - 2) bits: the header in byte at - 1, LEN in byte `at`
            b.store(b.noise(37), True, PADS[at % 3])
            s = b.stored[-1]
            assert s.in_at - 4 - seek == at and s.start_bit == 8 * (seek + at - 1) + 2
            out.append(b.case("window", "window/%s/%d" % (base, at), base=base, at=at, L=37, P=at - 2))
    return out


# ---- after: what the next block's first copy finds of a stored block ----------------------------------------------------------
def _after_case(name, Q, L, copies, history=b"", form=1):
    b = _Build(history)
    if Q:
        b.fixed(b.literals(Q, nine=Q // 3), False)
    b.store(b.noise(L), False, PADS[(L + Q) % 3])
    b.fixed([("M", n, d) for n, d in copies] + b.literals(3), True)
    return b.case("after", name, Q=Q, L=L, copies=list(copies), form=form, P=Q)


def _after():
    out = []
    for Q in AFTER_FRONT:
        for L in AFTER_LENS:
            for n in (3, 258):
                for D in after_distances(L, Q):
                    out.append(_after_case("after/%d/%d/%d/%d" % (Q, L, n, D), Q, L, [(n, D)]))
                # a far copy (its source comes back from memory, behind the flush) in front of a near one (from the ring)
                for far in sorted({d for d in (3839, 4097, min(32768, L + Q)) if 3839 <= d <= min(32768, L + Q)}):
                    for near in (1, 16):
                        out.append(_after_case("after2/%d/%d/%d/%d/%d" % (Q, L, n, far, near), Q, L, [(n, far), (3, near)], form=2))
                # 300 bytes of history in front of the stream: one byte and 300 bytes beyond everything the stream made
                for D in (L + Q + 1, L + Q + 300):
                    if D <= 32768:
                        out.append(_after_case("after3/%d/%d/%d/%d" % (Q, L, n, D), Q, L, [(n, D)], HISTORY[-300:], form=3))
    return out


# ---- chain: stored blocks back to back ----------------------------------------------------------------------------------------
CHAINS = {"0005": [0, 0, 0, 5], "big": [65535, 65535, 1], "ones": [1] * 300, "zeros": [0] * 300 + [7], "walk": list(LENS),
          "empty": [0], "empty-last": [5, 0]}
SHORT_CHAINS = ("0005", "empty", "empty-last")


def _chain():
    out = []
    for name, lens in CHAINS.items():
        b = _Build()
        for k, L in enumerate(lens):
            b.store(b.noise(L), k == len(lens) - 1)
        out.append(b.case("chain", "chain/" + name, lens=list(lens), P=0))
    return out


# ---- nlen: NLEN is not the complement of LEN ------------------------------------------------------------------------------------
def _nlen():
    out = []
    for off, nine in ((0, 6), (3, 1)):
        for L in (0, 5):
            pairs = [(L, (L ^ 0xffff) ^ (1 << k)) for k in range(16)] + [(L, L), (0, 0), (0xffff, 0xffff)]
            for ln, nl in sorted(set(pairs)):
                b = _Build()
                toks = b.literals(40, nine=nine)
                assert _nine_count(toks) == nine
                b.fixed(toks, False)
                front = bytes(b.plain)
                start = b.bits.bit_length()
                assert start % 8 == off
                b.bits.put(1, 1)
                b.bits.put(0, 2)
                b.bits.align()
                b.bits.put(ln, 16)
                b.bits.put(nl, 16)
                b.bits.out += b.noise(L + 8)                   # (bytes behind it: the decoder may not need them)
                out.append(Case("nlen", "nlen/%d/%d/%04x/%04x" % (off, L, ln, nl), b.bits.out, front, stored=[Stored(start, len(b.bits.out) - L - 8, 40, L, "zeros")],
                                off=off, L=L, len=ln, nlen=nl, P=40))
    return out


# ---- cuts: the input ends behind the stored header's byte -----------------------------------------------------------------------
def _cut_sources():
    return [c for c in _bit()] + [c for c in _len() if c.meta["L"] in CUT_LENS] + [c for c in _chain() if c.name[6:] in SHORT_CHAINS]


def cut_plain(c, cut):
    """what the first `cut` bytes of the case's stream hold: the blocks in front of the first stored block (complete: no cut
    lies in front of the byte behind its header's first bit), then every stored payload byte that is there behind a complete
    LEN / NLEN.  Only stored blocks may follow the first one up to `cut`."""
    n = c.stored[0].out_at
    for s in c.stored:
        if cut < s.in_at:
            break
        have = min(s.length, cut - s.in_at)
        n = s.out_at + have
        if have < s.length:
            break
    return c.plain[:n]


def _cuts():
    out = []
    for c in _cut_sources():
        first, lastb = c.stored[0], c.stored[-1]
        end = lastb.in_at + lastb.length                     # the stored blocks end here; a Huffman block behind them is never cut
        cuts = set()
        for cut in range(first.hdr_byte + 1, min(end + 1, len(c.stream))):
            inside = [s for s in c.stored if s.length > 64 and s.in_at < cut < s.in_at + s.length]
            if inside and cut - inside[0].in_at not in PAYLOAD_CUTS + (inside[0].length - 1,):
                continue
            cuts.add(cut)
        for cut in sorted(cuts):
            out.append(Case("cuts", "cuts/%s/%d" % (c.name, cut), c.stream[:cut], cut_plain(c, cut), stored=c.stored, of=c.name, cut=cut,
                            cap=len(c.plain), P=c.meta.get("P", 0)))
    return out


# ---- room: the output ends in or behind the stored block ------------------------------------------------------------------------
class Room:
    """one run: the case's stream with `cap` bytes of room; exact: the room is the whole plaintext (the run succeeds)"""

    def __init__(self, case, cap, kind):
        self.case, self.cap, self.kind, self.exact = case, cap, kind, cap == len(case.plain)


def _room_tail_case(L, P, tail):
    b = _Build()
    if P:
        b.fixed(b.literals(P, nine=P // 3), False)
    b.store(b.noise(L), False, PADS[(L + P) % 3])
    if tail == "stored":
        b.store(b"", True)
    else:
        b.fixed([], True)                                     # the end code alone
    return b.case("room", "room-tail/%d/%d/%s" % (L, P, tail), L=L, P=P, tail=tail)


@functools.lru_cache(maxsize=None)
def room_runs():
    out = []
    for c in cases("len"):
        L, P = c.meta["L"], c.meta["P"]
        if L:
            out += [Room(c, cap, "len") for cap in sorted({0, 1, P, P + 1, P + L - 1, P + L})]
    for L in (1, 16, 1024, 1025, 4096, 65535):
        for P in (0, 64, 65):
            for tail in ("stored", "eob"):
                c = _room_tail_case(L, P, tail)
                out.append(Room(c, len(c.plain), "tail"))
    for c in cases("after"):
        if c.meta["form"] == 1:
            n = c.meta["copies"][0][0]
            out.append(Room(c, c.meta["Q"] + c.meta["L"] + (1 if n == 3 else 131), "after"))    # inside the copy
    return out


_FAMILIES = {"len": _len, "bit": _bit, "window": _window, "after": _after, "chain": _chain, "nlen": _nlen, "cuts": _cuts}
VALID = ("len", "bit", "window", "after", "chain")


@functools.lru_cache(maxsize=None)
def cases(family):
    out = _FAMILIES[family]()
    assert len({c.name for c in out}) == len(out)
    return out


def valid_cases():
    return [c for f in VALID for c in cases(f)]


def totals():
    """family -> (streams, bytes of them); the room runs reuse the streams of `len` and `after`"""
    out = {f: (len(cases(f)), sum(len(c.stream) for c in cases(f))) for f in _FAMILIES}
    out["room"] = (len(room_runs()), sum(len(r.case.stream) for r in room_runs()))
    return out


# ---- one large stream of groups around stored blocks (part mode) -----------------------------------------------------------------
class Large:
    """comp: noise in front (lead), then the groups, then noise and a final stored block.  groups: how many; history: what
    precedes the output (lead=False: 32 KiB that the first groups' copies reach into); stored: a record per group's block"""


def stored_lookalike(s):
    """a byte 0 / 1 with LEN != 0 and NLEN = ~LEN behind it: the pattern the block-start finder takes for a stored block on a
    byte boundary, restated"""
    a = np.frombuffer(bytes(s), dtype=np.uint8)
    if a.size < 5:
        return False
    n = a.size - 4
    hit = ((a[:n] & 0xfe) == 0) & ((a[1:n + 1] | a[2:n + 2]) != 0) & ((a[1:n + 1] ^ a[3:n + 3]) == 0xff) & ((a[2:n + 2] ^ a[4:n + 4]) == 0xff)
    return bool(hit.any())


@functools.lru_cache(maxsize=None)
def large_stream(markers, tiny=0, lead=True):
    """groups of [sync marker if markers] [fixed block of literals] [stored block, its length from LENS in turn] [fixed block
    whose copies reach 1, L, L + 1 and up to 32768 bytes back, into earlier groups].  Without markers a short stored block
    follows every group's stored block: it begins on a byte boundary with a LEN that is not 0, which is the finder's pattern for
    a block start.  tiny: so many groups, of the lengths up to 49 only.  lead=False: no noise in front -- the first groups' copies
    reach into the 32 KiB that precede the stream."""
    b = _Build(b"" if lead else HISTORY)
    for _ in range(3 if lead else 0):
        b.store(b.noise(40000), False)
    lead_blocks = len(b.stored)
    lens = [L for L in LENS if L <= 49] if tiny else list(LENS)
    res = Large()
    res.groups, res.stored, k = 0, [], 0
    while (tiny and res.groups < tiny) or (not tiny and (k < len(lens) or len(b.bits.out) < (128 << 10) + 120000 * bool(lead))):
        L = lens[k % len(lens)]
        if markers:
            craft.stored_block(b.bits, b"", False)            # 00 00 ff ff on a byte boundary
        n = 1 + k % 9
        b.fixed(b.literals(n, nine=k % (n + 1)), False)     # the stored header comes at every bit offset in turn
        payload = b.noise(L)
        assert not stored_lookalike(payload)                  # (no start but the real ones: the part counts below are the groups')
        b.store(payload, False, PADS[k % 3])
        res.stored.append(b.stored[-1])
        if not markers:
            b.store(b.noise(33), False)
        made = len(b.history) + len(b.plain)
        copies = [(3, 1), (258, L), (4, L + 1), (258, 32768), (5, 20000 + 7 * k), (3, min(made, 32768)), (258, L + 33 + 1)]
        b.fixed([("M", n_, d) for n_, d in copies if 1 <= d <= min(made, 32768)] + [("L", k & 0xff)], False)
        res.groups += 1
        k += 1
    for _ in range(2):
        b.store(b.noise(40000), False)
    b.store(b"the end", True)
    res.comp, res.plain, res.history = bytes(b.bits.out), bytes(b.plain), b.history
    res.blocks = lead_blocks + 4 * res.groups + 3             # (a marker or the short stored block: four blocks a group either way)
    return res
