"""Valid raw deflate streams whose payload imitates block starts (test infrastructure).  Every large inflater trusts a
SEARCH for block starts: the two byte patterns of find_headers_range (inflate_large.hip) and zr_inflate_find_block
(inflate_host.cpp) -- 00 00 ff ff, and a byte 0 / 1 with LEN != 0 and NLEN = ~LEN behind it -- and a dynamic header that
passes F1 + F2.  A stored block carries its payload verbatim, so anyone can write a stream with thousands of such places
that are no block starts at all.  The streams here are that: a run of stored blocks (the carrier) whose filler bytes are
2..255 (none can begin either byte pattern), with decoys planted at chosen places of the payload, and in some streams
CPython level-6 text in front and behind, so that dynamic blocks (and the parts cut there) coexist with the decoys.

Decoy kinds (a stream's .kinds: kind -> the compressed byte every decoy of that kind begins at):
  marker        00 00 ff ff, filler behind it
  marker-dense  00 00 ff ff back to back: every 4 bytes a marker, a stored header with LEN = 0xff00 and one with LEN = 0xffff
  stored-chain  stored headers whose LEN lands exactly on the next one; the last one lands on filler, exactly on a genuine
                block start ("chain-on") or one byte in front of one ("chain-off")
  stored-far    stored headers with LEN from 1 to 65535 that end inside the stream, on filler
  dynamic       a complete dynamic header that the decoder accepts (the code sets of dynamic_cases.valid_cases() and
                zlib's own) at each of the 8 bit offsets, filler behind it
  expanding     a marker, a non-final fixed block of one literal and ('M', 258, 1) tokens (13 bits for 258 bytes: 159 per
                compressed byte, above kSlotRatio = 64, and long enough to pass the slot's slack as well), then an empty stored
                block -- whose 00 00 ff ff is the next marker, so the part runs out of its slot and, run again, lands on
                another decoy
  shadow        a marker and a complete FINAL fixed block of other text: a chain that enters it ends with status 1, a short
                length and wrong bytes -- which the sequential fallback cannot mask

pattern_candidates() restates the two byte patterns with the finder's conditions at the end of the stream, so the number
of candidates the device's pattern pass reports is a number the generator asserts; the count cells are the bounds of
inflate_large_plan.h and inflate_large_try, restated here (nothing is imported from the library).
Expected plaintext: CPython's zlib; the genuine blocks: inflate_util.oracle_block_starts."""
import functools
import zlib

import numpy as np

import deflate_craft as craft
import dynamic_cases as dc
import inflate_util
import synth

# ---- the plan's bounds, restated (inflate_large_plan.h, inflate_large_try) ----------------------------------------------------
PARTS_UNTHINNED = 12288                                   # kPartsUnthinned
SLOT_RATIO = 64                                           # kSlotRatio
SLOT_SLACK = 640 << 10                                    # kSlotSlack
MIN_LARGE = 128 << 10                                     # large_length_ok
RETRY_LIMIT = 1 << 30                                     # this file's own cap on what a stream's expanding decoys can demand
MARKER = b"\x00\x00\xff\xff"


def patterns_first(src_len):
    return min(src_len // 512 + 4096, 16384)


def cap2(src_len):
    return min(src_len // 512 + 4096, 8 << 20)


def retry_cap(part_bytes):                                # symbols
    return (part_bytes * 1032 + SLOT_SLACK + 7) & ~7


def pattern_candidates(comp):
    """(bytes b where 00 00 ff ff begins, bytes b where a stored header begins) as find_headers_range<true> takes them: b + 8 <
    src_len for both, b + 6 <= src_len for the marker, LEN != 0 and b + 5 + LEN <= src_len for the stored pattern.  The
    candidates are bit 8 (b + 4) for a marker and bit 8 b for a stored header."""
    a = np.frombuffer(bytes(comp), dtype=np.uint8)
    n = len(a)
    if n < 10:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    b = np.flatnonzero(a[:n - 8] <= 1).astype(np.int64)   # (b + 8 < n; the first byte is 0 or 1 in both patterns)
    v = [a[b + k].astype(np.int64) for k in range(5)]
    marker = (v[0] == 0) & (v[1] == 0) & (v[2] == 0xff) & (v[3] == 0xff) & (b + 6 <= n)
    ln = v[1] | (v[2] << 8)
    stored = (ln != 0) & ((v[1] ^ v[3]) == 0xff) & ((v[2] ^ v[4]) == 0xff) & (b + 5 + ln <= n)
    return b[marker], b[stored]


def candidate_bits(comp):
    """every pattern candidate's bit position, sorted (a marker and a stored header may name the same bit: both are listed)"""
    m, s = pattern_candidates(comp)
    return np.sort(np.concatenate([8 * (m + 4), 8 * s]))


def _stored(data, final=False):
    return bytes([1 if final else 0]) + len(data).to_bytes(2, "little") + (len(data) ^ 0xffff).to_bytes(2, "little") + bytes(data)


def _stored_header(length):
    return b"\x00" + length.to_bytes(2, "little") + (length ^ 0xffff).to_bytes(2, "little")


def _text_region(nbytes, seed):
    """level-6 deflate data of CPython that ends on a byte boundary and holds no final block"""
    text = synth.silesia_like(nbytes, seed=seed, seg_bytes=max(nbytes, 1 << 16)).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    return c.compress(text) + c.flush(zlib.Z_FULL_FLUSH)


def shadow_block(text):
    """marker + a complete FINAL fixed block of `text`"""
    b = craft.Bits()
    craft.fixed_block(b, [("L", x) for x in text], True)
    b.align()
    return MARKER + bytes(b.out)


def expanding_block(nbytes):
    """marker + a non-final fixed block of about `nbytes` bytes -- one literal, then ('M', 258, 1) -- + an empty stored block.
    Returns (bytes, the bytes the part behind the first marker decodes)."""
    reps = nbytes * 8 // 13
    b = craft.Bits()
    craft.fixed_block(b, [("L", 0x78)] + [("M", 258, 1)] * reps, False)
    craft.stored_block(b, b"", False)
    return MARKER + bytes(b.out), 1 + 258 * reps


def shifted(data, k, rng):
    """`data`'s bits from bit k of the first byte on; the k bits in front are random, and the bits behind it too"""
    v = (int.from_bytes(data, "little") << k) | int(rng.integers(0, 1 << k)) if k else int.from_bytes(data, "little")
    n = len(data) + (1 if k else 0)
    if k:
        v |= int(rng.integers(0, 1 << (8 - k))) << (8 * len(data) + k)
    return v.to_bytes(n, "little")


@functools.lru_cache(maxsize=None)
def dynamic_headers():
    """[(name, header bytes, header bits)]: complete dynamic headers (non-final, no symbol behind them) of crafted code sets of
    every header kind of dynamic_cases, and two that zlib wrote (with the codes that follow, cut after 160 bytes)"""
    out, seen = [], set()
    for c in dc.valid_cases():
        if c.kind in seen or c.name not in dc._SETS:
            continue
        seen.add(c.kind)
        b = craft.Bits()
        craft.dynamic_block(b, [], False, *dc._SETS[c.name], eob=False)
        nbits = b.bit_length()
        b.align()
        out.append((c.name, bytes(b.out), nbits))
    for seed in (1, 2):
        text = synth.silesia_like(60000, seed=0xD0 + seed, seg_bytes=1 << 16).tobytes()
        z = zlib.compressobj(6, zlib.DEFLATED, -15)
        comp = z.compress(text) + z.flush()
        assert comp[0] & 6 == 4                           # BTYPE = 2
        out.append(("zlib/%d" % seed, bytes([comp[0] & 0xfe]) + comp[1:160], 8 * 160))
    return out


class Stream:
    """name, comp, plain, kinds (see the module's docstring), count (pattern candidates: genuine stored headers + decoys),
    expanding [(compressed byte of the marker, bytes the decoy part decodes)], shadows [(byte of the marker, text)], lands
    {"chain-on" / "chain-off": (byte of the chain's last header, the byte its LEN ends on)}, region (first, last compressed
    byte of the stored carrier), dynamics [(byte, bit offset in it of the header)], retry_bound (bytes)"""

    @functools.cached_property
    def blocks(self):
        """(bit position of BFINAL, BTYPE) of every genuine block, as the oracle walks them"""
        status, blocks = inflate_util.oracle_block_starts(self.comp, len(self.plain) + 64)
        assert status == 1
        return blocks

    @property
    def genuine(self):
        """bit position of every genuine block (of its BFINAL bit)"""
        return [b for b, _ in self.blocks]

    @functools.cached_property
    def unfindable(self):
        """genuine stored blocks that no finder looks for: those that begin off a byte boundary and the empty ones (what a flush
        writes behind Huffman data) -- the stored pattern is a byte pattern and wants LEN != 0, F1 takes BTYPE = 2 alone --
        unless 00 00 ff ff ends where they begin.  The part in front decodes them; they are no part of their own."""
        n = 0
        for b, t in self.blocks:
            if t != 0:
                continue
            at = (b + 3 + 7) >> 3                         # LEN
            empty = self.comp[at:at + 2] == b"\x00\x00"
            behind_marker = b % 8 == 0 and self.comp[(b >> 3) - 4:b >> 3] == MARKER
            n += (b % 8 != 0 or empty) and not behind_marker and b != 0
        return n

    @functools.cached_property
    def genuine_ends(self):
        """every bit a genuine block ends on: the next block's start, and the end of the final one"""
        return set(self.genuine[1:]) | {8 * len(self.comp)}


class _Builder:
    def __init__(self, name, seed, blocks, head=0, tail=0):
        """blocks: the payload sizes of the stored carrier; head / tail: bytes of text for the level-6 regions around it"""
        self.name, self.rng = name, np.random.default_rng(seed)
        self.head = _text_region(head, seed + 1) if head else b""
        # (tail: bytes of text for a level-6 region, or the region itself: block data that ends on a byte boundary)
        self.tail = tail if isinstance(tail, bytes) else _text_region(tail, seed + 2) if tail else b""
        self.pay = []                                     # (first, one past the last) compressed byte of every payload
        at = len(self.head)
        for n in blocks:
            self.pay.append((at + 5, at + 5 + n))
            at += 5 + n
        self.carrier_end = at
        end = _stored(b"the end", True)
        self.total = at + len(self.tail) + len(end)
        buf = np.zeros(self.total, dtype=np.uint8)
        buf[:len(self.head)] = np.frombuffer(self.head, dtype=np.uint8)
        for lo, hi in self.pay:
            buf[lo - 5:lo] = np.frombuffer(_stored_header(hi - lo), dtype=np.uint8)
            buf[lo:hi] = self.rng.integers(2, 256, size=hi - lo, dtype=np.uint8)
        buf[at:at + len(self.tail)] = np.frombuffer(self.tail, dtype=np.uint8)
        buf[self.total - len(end):] = np.frombuffer(end, dtype=np.uint8)
        self.buf = buf
        self.used = np.zeros(self.total, dtype=bool)
        self.kinds, self.expanding, self.shadows, self.lands, self.dynamics = {}, [], [], {}, []
        self.cursor = (0, self.pay[0][0] + 64)            # sequential allocation: (payload, byte)

    def plant(self, at, data, kind):
        """`data` at compressed byte `at`: inside one payload, two filler bytes kept on either side of every decoy"""
        n = len(data)
        assert any(lo + 2 <= at and at + n + 2 <= hi for lo, hi in self.pay), (self.name, kind, at, n)
        assert not self.used[at - 2:at + n + 2].any(), (self.name, kind, at)
        self.buf[at:at + n] = np.frombuffer(bytes(data), dtype=np.uint8)
        self.used[at:at + n] = True
        self.kinds.setdefault(kind, []).append(at)
        return at

    def alloc(self, n, gap=96):
        """the next free place for n bytes, walking the payloads in order"""
        k, at = self.cursor
        while True:
            lo, hi = self.pay[k]
            at = max(at, lo + 2)
            if at + n + 2 <= hi and not self.used[at - 2:at + n + 2].any():
                self.cursor = (k, at + n + gap)
                return at
            if at + n + 2 > hi:
                k, at = k + 1, 0
                assert k < len(self.pay), (self.name, "no room left")
            else:
                at += 16

    # ---- the kinds ----
    def marker(self, at=None):
        return self.plant(self.alloc(4) if at is None else at, MARKER, "marker")

    def dense(self, reps):
        return self.plant(self.alloc(4 * reps), MARKER * reps, "marker-dense")

    def chain(self, n, kind="stored-chain", at=None, last_to=None):
        """n headers `00 01 00 fe ff X`, each landing on the next; the last one's LEN ends on `last_to` (default: 40 bytes on)"""
        at = self.alloc(6 * n + 48) if at is None else at
        data = b""
        for i in range(n - 1):
            data += _stored_header(1) + bytes([int(self.rng.integers(2, 256))])
        last = at + len(data)
        to = last + 5 + 40 if last_to is None else last_to
        assert 1 <= to - (last + 5) <= 65535
        data += _stored_header(to - (last + 5))
        self.plant(at, data, kind)
        if kind != "stored-chain":
            self.lands[kind] = (last, to)
        return at

    def far(self, length):
        at = self.alloc(5)
        assert at + 5 + length <= self.total - 64          # its end lies inside the stream
        return self.plant(at, _stored_header(length), "stored-far")

    def dynamic(self, header, k):
        data = shifted(header, k, self.rng)
        at = self.plant(self.alloc(len(data)), data, "dynamic")
        self.dynamics.append((at, k))
        return at

    def expand(self, nbytes, then_shadow=None):
        """then_shadow: the block behind the empty stored block's marker is a shadow's (a decoy chain of two links)"""
        data, produced = expanding_block(nbytes)
        tail = shadow_block(then_shadow)[4:] if then_shadow else b""
        at = self.plant(self.alloc(len(data) + len(tail)), data + tail, "expanding")
        self.expanding.append((at, produced))
        if then_shadow:
            self.kinds.setdefault("shadow", []).append(at + len(data) - 4)
            self.shadows.append((at + len(data) - 4, bytes(then_shadow)))
        return at

    def shadow(self, text, at=None):
        data = shadow_block(text)
        at = self.plant(self.alloc(len(data)) if at is None else at, data, "shadow")
        self.shadows.append((at, bytes(text)))
        return at

    def block_end_chains(self):
        """a chain whose last LEN lands exactly on a genuine block start, and one that lands a single byte in front of one"""
        for kind, k, off in (("chain-on", 1, 0), ("chain-off", 2, 1)):
            hi = self.pay[k][1]                           # the next block's header begins here
            self.chain(10, kind, at=hi - 6 * 10 - 200, last_to=hi - off)

    def count(self):
        m, s = pattern_candidates(self.buf.tobytes())
        return len(m) + len(s)

    def top_up(self, cell):
        """single markers, spread over the free filler of the carrier, until the stream has `cell` pattern candidates"""
        need = cell - self.count()
        assert need >= 0, (self.name, cell, need)
        free = [(lo + 8, hi - 8) for lo, hi in self.pay]
        room = sum(hi - lo for lo, hi in free)
        stride = max(12, (room - int(self.used.sum())) // (need + 2 * len(free) + 8)) if need else 0
        placed, k, at = 0, 0, free[0][0]
        while placed < need:
            lo, hi = free[k]
            if at + 8 > hi:
                k += 1
                assert k < len(free), (self.name, "no room for the markers", placed, need)
                at = free[k][0]
                continue
            if self.used[at - 2:at + 6].any():
                at += 8
                continue
            self.plant(at, MARKER, "marker")
            placed += 1
            at += stride
        assert self.count() == cell, (self.name, self.count(), cell)

    def finish(self):
        s = Stream()
        s.name, s.comp = self.name, self.buf.tobytes()
        z = zlib.decompressobj(-15)
        s.plain = z.decompress(s.comp)
        assert z.eof and not z.unused_data
        s.kinds, s.expanding, s.shadows, s.lands, s.dynamics = self.kinds, self.expanding, self.shadows, self.lands, self.dynamics
        s.region = (self.pay[0][0] - 5, self.carrier_end)
        s.count = self.count()
        bits = candidate_bits(s.comp)
        s.retry_bound = 0
        for at, _ in s.expanding:                         # the room its decoy part can ask for when it runs again
            nxt = bits[np.searchsorted(bits, 8 * (at + 4), side="right")]
            s.retry_bound += 2 * retry_cap((int(nxt) - 8 * (at + 4) + 7) >> 3)
        assert s.retry_bound <= RETRY_LIMIT, (s.name, s.retry_bound)
        assert MIN_LARGE <= len(s.comp), (s.name, len(s.comp))
        return s


_SHADOW_TEXT = b"shadow text: a chain that lands here ends the stream early, with bytes nobody compressed. " * 3


def _mixed(b, dyn_every=1):
    """some of every sparse kind"""
    b.block_end_chains()
    # a shadow as the FIRST candidate behind a genuine block start: a chain that takes "the next start" for "the start the
    # part ended on" walks into it
    b.shadow(_SHADOW_TEXT[:50], at=b.pay[1][0] + 2)
    for _ in range(4):
        b.marker()
    b.chain(2)
    b.chain(10)
    for length in (1, 2, 257, 4096, 65535):
        b.far(length)
    for i, (_, hdr, _) in enumerate(dynamic_headers()[::dyn_every]):
        b.dynamic(hdr, i % 8)
    b.shadow(_SHADOW_TEXT)
    b.shadow(_SHADOW_TEXT[:40])


@functools.lru_cache(maxsize=None)
def small(name):
    """the streams between 128 KiB and 1 MiB"""
    if name in ("c63", "c64"):                            # 63: F1 + F2 run (the patterns do not cut); 64: the patterns alone
        b = _Builder(name, 0xDEC0 + int(name[1:]), [50000, 60000, 65535, 30000])
        _mixed(b, dyn_every=2)
        b.top_up(int(name[1:]))
    elif name == "chains":
        b = _Builder(name, 0xDEC2, [65535] * 5 + [1234])
        _mixed(b)
        b.chain(1000)
        for k in range(8):                                # every dynamic header at every bit offset
            for _, hdr, _ in dynamic_headers():
                b.dynamic(hdr, k)
    elif name == "expanding":
        b = _Builder(name, 0xDEC3, [65535] * 5 + [4000])
        b.block_end_chains()
        b.shadow(_SHADOW_TEXT[:50], at=b.pay[1][0] + 2)
        for k in range(6):
            b.expand(8000 + 500 * k)
            b.shadow(_SHADOW_TEXT[:60 + k])
        b.expand(9000, then_shadow=_SHADOW_TEXT)           # ... and one that lands on a shadow at once
    elif name == "dense":                                 # stays under kPartsUnthinned
        b = _Builder(name, 0xDEC4, [65535] * 7 + [999])
        _mixed(b, dyn_every=3)
        b.dense(1000)
    elif name == "dense-wide":                            # far more candidates than cap2: the device path declines
        b = _Builder(name, 0xDEC5, [65535] * 12)
        b.dense(12000)
        b.shadow(_SHADOW_TEXT)
    elif name == "steep":
        # a GENUINE block of 159 symbols per byte behind the carrier (a sync marker in front of it, so it is a part of its
        # own): the part on the chain overflows its slot, among the 2000 decoy headers of a dense run that promise 65280
        # bytes each -- in a piece those put the stream over its retry cap, and the chain's own full part must still run again
        b = _Builder(name, 0xDEC7, [65535] * 6 + [777], tail=_stored(b"") + expanding_block(20000)[0][4:])
        _mixed(b, dyn_every=3)
        b.dense(1000)
    elif name == "cut-short":
        # a marker two bytes behind EVERY genuine header: each genuine part has a few bytes to its next start, so in a piece
        # (whose slack is small) each of the 25 overflows its slot -- more full parts on the chain than a piece over its
        # retry cap (the dense run sees to that) runs again one by one
        b = _Builder(name, 0xDEC9, [20000] * 24 + [500])
        for lo, _ in b.pay:
            b.marker(at=lo + 2)
        b.dense(1000)
    elif name == "text":                                  # level-6 text in front and behind
        b = _Builder(name, 0xDEC6, [65535, 40000, 65535], head=900000, tail=600000)
        _mixed(b)
        b.chain(1000)
        b.top_up(2000)
    else:
        raise KeyError(name)
    s = b.finish()
    assert len(s.comp) <= (1 << 20), (name, len(s.comp))
    return s


SMALL = ("c63", "c64", "chains", "expanding", "dense", "steep", "cut-short", "dense-wide", "text")


def _carrier_blocks():
    rng = np.random.default_rng(0xCA44)
    sizes = []
    while sum(sizes) + 5 * len(sizes) < (8 << 20):
        sizes.append(int(rng.integers(20000, 65536)))
    return sizes


LARGE = ("unthinned", "unthinned+1", "first", "first+1", "cap2", "cap2+1")


def large_cell(name, src_len):
    return {"unthinned": PARTS_UNTHINNED, "unthinned+1": PARTS_UNTHINNED + 1, "first": patterns_first(src_len),
            "first+1": patterns_first(src_len) + 1, "cap2": cap2(src_len), "cap2+1": cap2(src_len) + 1}[name]


@functools.lru_cache(maxsize=None)
def large(name):
    """ONE carrier of 8 MiB (the same blocks, filler and sparse decoys) with markers up to the cell's count"""
    b = _Builder("8m/" + name, 0xDEC8, _carrier_blocks())
    _mixed(b)
    b.chain(1000)
    assert b.total > (6 << 20) and patterns_first(b.total) < cap2(b.total)
    b.top_up(large_cell(name, b.total))
    return b.finish()


def cut_inside_a_decoy(s):
    """a compressed byte inside a decoy with complete blocks in front of it, where a test may cut the stream"""
    if "chain-off" in s.lands:
        return s.lands["chain-off"][0] + 3                # inside the header that lands one byte in front of a genuine start
    return sorted(at for v in s.kinds.values() for at in v)[0] + 4 * 6000 + 2


def get(name):
    return small(name) if name in SMALL else large(name)


ALL = SMALL + LARGE


def benign(nbytes, seed=0xBE9):
    """a stored carrier of the same build without a single decoy: nothing but its genuine headers passes the patterns"""
    sizes, rng = [], np.random.default_rng(seed)
    while sum(sizes) + 5 * len(sizes) < nbytes:
        sizes.append(int(rng.integers(20000, 65536)))
    return _Builder("benign/%d" % nbytes, seed, sizes).finish()
