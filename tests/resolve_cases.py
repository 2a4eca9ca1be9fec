"""Token streams for the inflate copy-resolution kernels (inflate_resolve.hip), built token by token (test infrastructure).

A Builder takes literal bytes and (length, distance) matches and emits the arrays of include/zng_rocm.h as the device stage
reads them: `tokens` (uint32: a literal-run count, or 0x80000000 | (len - 3) << 16 | (dist - 1)), `literals`, and `segs`,
nsegs + 1 triples {first token, first output byte, first literal}.  Two cut policies, both inside the contract (every segment
but the last holds >= 32768 and < 32768 + 258 bytes):
  "decoder"  what inflate_host.cpp does: a segment closes at the first token boundary at or past 32768, and a literal run is
             split so that it ends a segment at exactly 32768;
  "placed"   the case chooses every segment's size in 32768 .. 33025, and ends the segment with a match that starts in front
             of byte 32768.
replay() is the expected plaintext: a bytearray, slices and pattern repetition -- no segments, symbols or rings.
check_contract() is what every array must pass before it goes to the GPU: the device stage has no error channel.

The Builder also tracks where K1's flush mark stands (`flushed += 2048` whenever `op - flushed >= 2048`, looked at when a
token and when a chunk of a literal run begins).  That is used to PLACE copies, never to predict a byte."""
import functools
import itertools

import numpy as np

CTX = 32768
SEG_END = CTX + 258                                 # a segment holds fewer bytes than this
MATCH = 0x80000000
FLUSH, LITWIN = 2048, 1024                          # K1: symbols per flush, bytes of the literal window


class ContractError(AssertionError):
    pass


def tok_match(length, dist):
    return MATCH | ((length - 3) << 16) | (dist - 1)


def replay(tokens, literals, window=b""):
    """the bytes the token list produces behind `window`"""
    buf = bytearray(window)
    lit = bytes(literals) if not isinstance(literals, np.ndarray) else literals.tobytes()
    lp = 0
    for tok in (tokens.tolist() if isinstance(tokens, np.ndarray) else tokens):
        if tok >> 31:
            n, dist = ((tok >> 16) & 0xff) + 3, (tok & 0xffff) + 1
            at = len(buf) - dist
            if at < 0:
                raise ValueError("distance %d with %d bytes behind it" % (dist, len(buf)))
            if dist >= n:
                buf += buf[at:at + n]
            else:
                buf += (buf[at:] * (n // dist + 1))[:n]
        else:
            buf += lit[lp:lp + tok]
            lp += tok
    if lp != len(lit):
        raise ValueError("the runs take %d literals, the array holds %d" % (lp, len(lit)))
    return bytes(buf[len(window):])


def token_spans(tokens):
    """per token: is it a match, how many bytes it produces, output offset in front of it, literals in front of it"""
    t = np.asarray(tokens, dtype=np.uint32).astype(np.int64)
    is_match = (t >> 31) != 0
    n = np.where(is_match, ((t >> 16) & 0xff) + 3, t)
    out0 = np.concatenate(([0], np.cumsum(n)))
    lit0 = np.concatenate(([0], np.cumsum(np.where(is_match, 0, n))))
    return is_match, n, out0, lit0


def check_contract(case, window_len=None):
    """raise ContractError("<rule>: ...") unless the arrays are ones the device stage may be given.  Rules: segs (shape and
    agreement with the tokens), segment size, encoding, distance above 32768, distance too far back, literal total."""
    tokens = np.asarray(case.tokens)
    segs = np.asarray(case.segs)
    wl = len(case.window) if window_len is None else int(window_len)
    if tokens.dtype != np.uint32 or segs.dtype != np.uint64 or np.asarray(case.literals).dtype != np.uint8:
        raise ContractError("encoding: tokens are uint32, literals uint8, segs uint64")
    if segs.ndim != 1 or segs.size % 3 or segs.size < 6:
        raise ContractError("segs: not nsegs + 1 triples")
    tri = segs.reshape(-1, 3).astype(np.int64)
    is_match, n, out0, lit0 = token_spans(tokens)
    t = tokens.astype(np.int64)
    if (is_match & ((t >> 24) & 0x7f != 0)).any():
        raise ContractError("encoding: bits 24..30 of a match are not zero")
    if (~is_match & (t == 0)).any():
        raise ContractError("encoding: a literal run of no bytes")
    dist = (t & 0xffff) + 1
    if (is_match & (dist > CTX)).any():
        raise ContractError("distance above 32768 at token %d" % int(np.argmax(is_match & (dist > CTX))))
    far = is_match & (dist > out0[:-1] + wl)
    if far.any():
        k = int(np.argmax(far))
        raise ContractError("distance too far back: token %d names %d bytes back with %d in front of it"
                            % (k, int(dist[k]), int(out0[k]) + wl))
    if int(lit0[-1]) != len(case.literals):
        raise ContractError("literal total: the runs take %d, the array holds %d" % (int(lit0[-1]), len(case.literals)))
    if tuple(tri[0]) != (0, 0, 0) or tuple(tri[-1]) != (tokens.size, int(out0[-1]), len(case.literals)):
        raise ContractError("segs: first triple is not zero or the terminal triple does not close the arrays")
    if (np.diff(tri[:, 0]) < 0).any() or tri[-1, 0] > tokens.size:
        raise ContractError("segs: token indices go backwards")
    if (out0[tri[:, 0]] != tri[:, 1]).any() or (lit0[tri[:, 0]] != tri[:, 2]).any():
        raise ContractError("segs: a triple disagrees with the tokens in front of it")
    size = np.diff(tri[:, 1])
    if (size[:-1] < CTX).any() or (size >= SEG_END).any():
        k = int(np.argmax((size < CTX) | (size >= SEG_END))) if (size >= SEG_END).any() else int(np.argmax(size[:-1] < CTX))
        raise ContractError("segment size: segment %d holds %d bytes" % (k, int(size[k])))
    if int(case.out_len) != int(out0[-1]):
        raise ContractError("segs: out_len is not what the tokens produce")


class Stream:
    """one token stream as the ABI's arrays, its window, and the output ranges [(name, first, end)] its cases cover"""

    def __init__(self, name, tokens, literals, segs, window=b"", marks=()):
        self.name = name
        self.tokens = np.ascontiguousarray(tokens, dtype=np.uint32)
        self.literals = np.ascontiguousarray(literals, dtype=np.uint8)
        self.segs = np.ascontiguousarray(segs, dtype=np.uint64).reshape(-1)
        self.window = bytes(window)
        self.marks = list(marks)
        self._plain = None

    @property
    def nsegs(self):
        return self.segs.size // 3 - 1

    @property
    def out_len(self):
        return int(self.segs[-2])

    def seg_bounds(self):
        return self.segs.reshape(-1, 3)[:, 1].astype(np.int64)

    def expected(self):
        if self._plain is None:
            self._plain = replay(self.tokens, self.literals, self.window)
        return self._plain

    def describe(self, off):
        """where output byte `off` lies: case name and offset within the case, segment and offset within the segment"""
        o = self.seg_bounds()
        s = int(np.searchsorted(o, off, side="right")) - 1
        s = min(max(s, 0), self.nsegs - 1)
        where = "segment %d + %d (of %d, tail from %d)" % (s, off - int(o[s]), int(o[s + 1] - o[s]), int(o[s + 1] - o[s]) - CTX)
        inside = [m for m in self.marks if m[1] <= off < m[2]]
        before = [m for m in self.marks if m[2] <= off]
        if inside:
            where = "case %s + %d, %s" % (inside[-1][0], off - inside[-1][1], where)
        elif before:
            where = "%d bytes behind case %s, %s" % (off - before[-1][2], before[-1][0], where)
        return "%s: byte %d, %s" % (self.name, off, where)

    def first_mismatch(self, got):
        """None when `got` is the expected plaintext, else a description of the first byte that differs"""
        want = self.expected()
        if got == want:
            return None
        if len(got) != len(want):
            return "%s: %d bytes instead of %d" % (self.name, len(got), len(want))
        a, b = np.frombuffer(got, dtype=np.uint8), np.frombuffer(want, dtype=np.uint8)
        off = int(np.argmax(a != b))
        return "%s (got %d, expected %d; %d bytes differ)" % (self.describe(off), a[off], b[off], int((a != b).sum()))

    def prefix(self, nsegs, last_tokens=None, name=None):
        """the first nsegs segments; of the last of them only its first `last_tokens` tokens (None: all)"""
        tri = self.segs.reshape(-1, 3)
        assert 1 <= nsegs <= self.nsegs
        t_end = int(tri[nsegs, 0])
        if last_tokens is not None:
            t_end = min(t_end, int(tri[nsegs - 1, 0]) + last_tokens)
        _, _, out0, lit0 = token_spans(self.tokens[:t_end])
        segs = np.concatenate((tri[:nsegs].reshape(-1), np.array([t_end, out0[-1], lit0[-1]], dtype=np.uint64)))
        marks = [m for m in self.marks if m[2] <= int(out0[-1])]
        s = Stream(name or "%s[:%d]" % (self.name, nsegs), self.tokens[:t_end], self.literals[:int(lit0[-1])], segs,
                   self.window, marks)
        if self._plain is not None:
            s._plain = self._plain[:int(out0[-1])]
        return s

    def extended(self, tokens, literals=b"", name=None):
        """the stream with more tokens in its last segment"""
        toks = np.concatenate((self.tokens, np.asarray(tokens, dtype=np.uint32)))
        lits = np.concatenate((self.literals, np.frombuffer(bytes(literals), dtype=np.uint8)))
        _, _, out0, lit0 = token_spans(toks)
        segs = self.segs.copy()
        segs[-3:] = (toks.size, out0[-1], lit0[-1])
        return Stream(name or self.name + "+", toks, lits, segs, self.window, self.marks)

    def craft_tokens(self):
        """the same token list for tests/deflate_craft.py: ("L", byte) and ("M", length, distance)"""
        out, lp, lit = [], 0, self.literals.tolist()
        for tok in self.tokens.tolist():
            if tok >> 31:
                out.append(("M", ((tok >> 16) & 0xff) + 3, (tok & 0xffff) + 1))
            else:
                out += [("L", v) for v in lit[lp:lp + tok]]
                lp += tok
        return out


class Builder:
    def __init__(self, policy="decoder", sizes=None, window=b""):
        assert policy in ("decoder", "placed")
        self.policy = policy
        self.window = bytes(window)
        self.sizes = itertools.cycle(sizes) if sizes is not None else None
        assert (policy == "placed") == (sizes is not None)
        self.tokens, self.lits, self.segs, self.marks = [], bytearray(), [(0, 0, 0)], []
        self.out = self.seg0 = 0
        self._new_segment_state()

    def _new_segment_state(self):
        self.cut = next(self.sizes) if self.sizes is not None else CTX
        assert CTX <= self.cut < SEG_END
        self.flushed = self.lit_seen = self.lit_base = 0          # K1's state, for placing copies only

    @property
    def op(self):
        """bytes the current segment holds"""
        return self.out - self.seg0

    def room(self):
        return self.cut - self.op

    def mark_at_next_token(self):
        """K1's flush mark while the NEXT token is resolved (it is moved when a token begins)"""
        return self.flushed + (FLUSH if self.op - self.flushed >= FLUSH else 0)

    def _close(self):
        self.segs.append((len(self.tokens), self.out, len(self.lits)))
        self.seg0 = self.out
        self._new_segment_state()

    def _token_begins(self):
        if self.op >= self.cut:
            assert self.policy == "decoder" or self.op == self.cut
            self._close()
        if self.op - self.flushed >= FLUSH:
            self.flushed += FLUSH

    def lit(self, data):
        """one literal-run token; cut where a segment has to end (as the decoder cuts its runs)"""
        data = bytes(data)
        while data:
            self._token_begins()
            n = min(len(data), self.room())
            self.tokens.append(n)
            self.lits += data[:n]
            data = data[n:]
            while n:                                              # K1's chunks of a run
                if self.op - self.flushed >= FLUSH:
                    self.flushed += FLUSH
                avail = self.lit_base + LITWIN - self.lit_seen
                if avail == 0:
                    self.lit_base, avail = self.lit_seen, LITWIN
                c = min(n, avail, FLUSH)
                self.out += c
                self.lit_seen += c
                n -= c

    def match(self, length, dist):
        self._token_begins()
        assert 3 <= length <= 258 and 1 <= dist <= CTX and dist <= self.out + len(self.window), (length, dist, self.out)
        assert self.policy == "decoder" or self.op + length <= self.cut, "a placed segment ends exactly at its size"
        self.tokens.append(tok_match(length, dist))
        self.out += length

    def fill(self, rng, n):
        """n random literal bytes in one token"""
        if n:
            self.lit(rng.integers(0, 256, size=n, dtype=np.uint8).tobytes())

    def fill_to(self, rng, op):
        assert self.op <= op, (self.op, op)
        self.fill(rng, op - self.op)

    def filler(self, rng, n):
        """n bytes of filler: random literals; with 32 KiB of history, a short run and then copies of earlier bytes from
        random places (as random to look at, and a fiftieth of the tokens)"""
        if n >= 600 and self.out + len(self.window) >= CTX:
            self.fill(rng, 19)
            n -= 19
            while n >= 300:
                self.match(258, int(rng.integers(258, CTX + 1)))
                n -= 258
        self.fill(rng, n)

    def pad_segment(self, rng, literal=False):
        """filler (literal=True: one run of literals) up to the segment's end; a placed segment above 32768 ends in a match
        from in front of 32768"""
        if self.op >= self.cut:
            return
        filler = self.fill if literal else self.filler
        if self.cut == CTX:
            filler(rng, self.room())
            return
        lo, hi = max(self.op, self.cut - 258), min(CTX - 1, self.cut - 3)
        assert lo <= hi, "too late in a placed segment to end it with a match"
        at = int(rng.integers(lo, hi + 1))
        filler(rng, at - self.op)
        n = self.cut - at
        self.match(n, int(rng.integers(1, min(CTX, self.out + len(self.window)) + 1)))

    def open_segment(self):
        """close a full segment now (the next token would): afterwards op is what the next token finds"""
        if self.op >= self.cut:
            assert self.policy == "decoder" or self.op == self.cut
            self._close()

    def lens_to_end(self, rng):
        """random match lengths that end the segment as the policy ends it"""
        if self.policy == "decoder":
            draw = rng.integers(3, 259, size=self.room() // 3 + 1)
            return draw[:int(np.searchsorted(np.cumsum(draw), self.room(), side="left")) + 1].tolist()
        lo, hi = max(self.op, self.cut - 258), min(CTX - 1, self.cut - 3)
        ok = [at for at in range(lo, hi + 1) if at - self.op not in (1, 2)]
        last_from = ok[int(rng.integers(0, len(ok)))]
        return _lens_to(rng, last_from - self.op) + [self.cut - last_from]

    def matches_to_end(self, rng):
        for n in self.lens_to_end(rng):
            self.match(n, int(rng.integers(1, min(CTX, self.out + len(self.window)) + 1)))

    def mark(self, name, first, end=None):
        self.marks.append((name, first, self.out if end is None else end))

    def finish(self, name):
        if self.policy == "decoder" and self.op >= self.cut:
            self._close()               # the decoder opens the next segment as soon as a token fills one: an empty last segment
        segs = np.array(self.segs + [(len(self.tokens), self.out, len(self.lits))], dtype=np.uint64)
        return Stream(name, np.array(self.tokens, dtype=np.uint32), np.frombuffer(bytes(self.lits), dtype=np.uint8), segs,
                      self.window, self.marks)


PLACED_SIZES = (32769, 32768, 32775, 32776, 33025)      # by segment index mod 5: 32768 never falls on 63..65 or 127..129


def _builder(policy, window=b""):
    return Builder(policy, PLACED_SIZES if policy == "placed" else None, window)


# ---- (a) K1: positions against the flush mark ---------------------------------------------------------------------------
def _flush_requests(F):
    """[(op relative to F, length, distance, name)]: copies resolved while the flush mark stands at F"""
    req = []
    for ln in (3, 64, 65, 258):
        # dist >= len: the source [src, src + ln) ends below F, ends at F, straddles F, starts at F - 1, starts at F
        for tag, src in (("below", F - ln - 5), ("ends_at", F - ln), ("straddles", F - (ln + 1) // 2), ("from_F-1", F - 1),
                         ("from_F", F)):
            rel = max(src + ln - F, 0) + 40
            req.append((rel, ln, F + rel - src, "F%d_far_len%d_%s" % (F, ln, tag)))
        # the first token behind the flush: every source symbol was stored a moment ago
        req.append((0, ln, ln, "F%d_far_len%d_at_mark_ends_at" % (F, ln)))
        req.append((0, ln, ln + 5, "F%d_far_len%d_at_mark_below" % (F, ln)))
        # dist == 1: the source symbol is F - 1 (read back) or F (ring); it cannot lie further below a mark the copy is behind
        for k in (0, 1):
            req.append((k, ln, 1, "F%d_run_len%d_src_F%+d" % (F, ln, k - 1)))
    for d in (2, 3, 63, 64, 65, 127, 257):
        for ln in sorted({d + 1, 65, 258}):
            if ln <= d or ln > 258:
                continue
            # overlapped: the source is [op - d, op) and op >= F, so it ends at F (op = F), straddles F, starts at F - 1 or at F
            for k in sorted({0, d // 2, d - 1, d}):
                req.append((k, ln, d, "F%d_overlap_dist%d_len%d_op_F+%d" % (F, d, ln, k)))
    return req


def _sweep(req, limit):
    """the requests as lists that can follow each other inside one flush window / one segment"""
    left, rows = sorted(req, key=lambda r: (r[0], r[1])), []
    while left:
        cur, row, rest = 0, [], []
        for r in left:
            if r[0] >= cur and r[0] + r[1] <= limit:
                row.append(r)
                cur = r[0] + r[1]
            else:
                rest.append(r)
        assert row, left[0]
        rows.append(row)
        left = rest
    return rows


def flush_mark_stream(policy="decoder", seed=0xA1):
    rng = np.random.default_rng(seed)
    b = _builder(policy)
    rows = {F: _sweep(_flush_requests(F), FLUSH - 1) for F in (2048, 4096, 6144)}
    for k in range(max(len(r) for r in rows.values())):
        b.open_segment()
        for F in (2048, 4096, 6144):
            if k >= len(rows[F]):
                continue
            for rel, ln, dist, name in rows[F][k]:
                b.fill_to(rng, F + rel)
                assert b.mark_at_next_token() == F, (name, b.op, b.flushed)
                at = b.out
                b.match(ln, dist)
                b.mark(name, at)
        b.pad_segment(rng)
    # literal runs that begin with 2046, 2047 or 2048 symbols unflushed, then copies out of the oldest unflushed symbols
    for unflushed in (2046, 2047, 2048):
        for run in (1, 2047, 2048, 2049, 4096, 5000):
            if b.room() < 12000:
                b.pad_segment(rng)
                b.fill(rng, 1)
            for _ in range(6):
                gap = b.op - b.flushed
                if gap == unflushed:
                    break
                b.fill(rng, unflushed - gap if gap < unflushed else 1 if gap >= FLUSH else FLUSH - gap)
            assert b.op - b.flushed == unflushed
            at = b.out
            b.fill(rng, run)
            m = b.mark_at_next_token()
            b.match(65, b.op - m or 65)                # from the oldest unflushed symbol on (none left: the last 65 stored)
            b.match(3, b.op - (b.mark_at_next_token() - 1))      # ... and from the symbol in front of the mark
            b.match(258, b.op - max(b.mark_at_next_token() - 100, 0))
            b.mark("unflushed%d_run%d" % (unflushed, run), at)
    return b.finish("flush_mark/" + policy)


# ---- (b) K1: the previous segment ---------------------------------------------------------------------------------------
def _prev_requests():
    """[(op, length, distance, name)]: copies in the first bytes of a segment that reach into the 32 KiB in front of it"""
    req = []
    for d in (1, 2, 3, 64, 257, 258, 300, CTX):
        for op in sorted({0, 1, d - 1, d, d + 1}):
            for ln in sorted({3, 258} | ({d + 1} if 3 <= d + 1 <= 258 else set())):
                if op + ln <= CTX:
                    req.append((op, ln, d, "prev_dist%d_len%d_op%d" % (d, ln, op)))
    return req


def previous_segment_stream(policy="decoder", window_len=0, seed=0xB2):
    rng = np.random.default_rng(seed)
    window = rng.integers(0, 256, size=window_len, dtype=np.uint8).tobytes()
    b = _builder(policy, window)
    if window_len < CTX:
        b.pad_segment(rng)                              # nothing in front of segment 0 that all of these could reach
    for row in _sweep(_prev_requests(), CTX if policy == "decoder" else CTX - 300):
        if b.op:
            b.pad_segment(rng)
        b.open_segment()
        for op, ln, dist, name in row:
            b.fill_to(rng, op)
            at = b.out
            b.match(ln, dist)
            b.mark(name, at)
    b.pad_segment(rng)
    b.fill(rng, 5)
    return b.finish("previous_segment/%s/w%d" % (policy, window_len))


# ---- (c) K1: literal window and token batches ---------------------------------------------------------------------------
def literal_window_stream(policy="decoder", seed=0xC3):
    rng = np.random.default_rng(seed)
    b = _builder(policy)
    b.pad_segment(rng)
    # a segment's first literal at every phase mod 16: each of these segments takes 17 literals, the rest are matches
    for k in range(17):
        b.open_segment()
        at = b.out
        b.fill(rng, 17)
        b.matches_to_end(rng)
        b.mark("first_literal_phase_step%d" % k, at)
    # runs that end exactly on, begin exactly on, and cross a multiple of 1024 literals from the segment's first
    b.open_segment()
    at = b.out
    for run in (1000, 24, 7, 1017 + 1024, 3, 1021, 1024, 2048, 1, 1023, 1025, 1023, 4096, 5, 3000):
        b.fill(rng, run)
        b.match(4, int(rng.integers(1, 2000)))
    b.mark("runs_against_the_literal_window", at)
    b.pad_segment(rng)
    # segments of exactly 1 (a single 32768-literal token), 63, 64, 65, 128 and 129 tokens
    for ntok in (1, 63, 64, 65, 128, 129):
        b.open_segment()
        n_end = 1 if b.cut == CTX else 2                # pad_segment: a literal run, and the match that ends a placed segment
        if ntok < n_end:
            continue
        at, t0 = b.out, len(b.tokens)
        for j in range(ntok - n_end):
            if (j + ntok - n_end) % 2:                  # alternating, and a match is the last of them
                b.fill(rng, 100 + j)
            else:
                b.match(3 + (7 * j) % 256, int(rng.integers(1, CTX + 1)))
        b.pad_segment(rng, literal=True)
        assert len(b.tokens) - t0 == ntok, (ntok, len(b.tokens) - t0)
        b.mark("segment_of_%d_tokens" % ntok, at)
    # one segment of matches only
    b.open_segment()
    at = b.out
    b.matches_to_end(rng)
    b.mark("matches_only", at)
    b.open_segment()
    b.fill(rng, 3)
    return b.finish("literal_window/" + policy)


def last_literals_streams(seed=0xC4):
    """17 streams whose last segment ends in a run of 1 .. 17 literals, the last bytes of `literals`"""
    out = []
    for k in range(1, 18):
        rng = np.random.default_rng(seed + k)
        b = _builder("decoder")
        b.fill(rng, 20000)
        while b.room() > 300:
            b.match(258, int(rng.integers(1, 20000)))
        b.pad_segment(rng)
        b.match(100, CTX)
        at = b.out
        b.fill(rng, k)
        b.mark("last_run_of_%d" % k, at)
        out.append(b.finish("last_literals/%d" % k))
    return out


# ---- (d) K2 and K3: alive streams ---------------------------------------------------------------------------------------
def _lens_to(rng, n):
    """match lengths (3 .. 258 each) that add up to exactly n (n == 0 or n >= 3)"""
    if n == 0:
        return []
    assert n >= 3
    draw = rng.integers(3, 259, size=n // 3 + 1)
    c = np.cumsum(draw)
    k = int(np.searchsorted(c, n - 3, side="right"))          # draws that leave at least 3 bytes
    lens = draw[:k].tolist()
    rem = n - (int(c[k - 1]) if k else 0)
    return lens + ([rem] if rem <= 258 else [rem - 3, 3])


def alive_stream(policy, window_len, nsegs, seed=0xD4):
    """32768 random bytes (or a random window and no literals at all), then matches only, every distance drawn from about
    [32768 - 300, 32768]: every byte descends from the first 32 KiB on a path of its own, every tail symbol stays a
    reference until the chain reaches the front, and the plaintext has no period.  nsegs full segments and a short one."""
    rng = np.random.default_rng(seed + 1000 * window_len + (1 if policy == "placed" else 0))
    window = rng.integers(0, 256, size=window_len, dtype=np.uint8).tobytes()
    b = _builder(policy, window)
    if window_len == 0:
        if policy == "decoder":
            b.fill(rng, CTX)
        else:
            b.pad_segment(rng)
    for s in range(nsegs + 1):
        b.open_segment()
        lens = b.lens_to_end(rng)
        jitter = rng.integers(0, 301, size=len(lens)).tolist()
        for n, back in zip(lens, jitter):
            b.match(n, max(1, min(CTX, b.out + window_len) - back))
    return b.finish("alive/%s/w%d" % (policy, window_len))


ALIVE_NSEGS = (1, 2, 3, 64, 65, 66, 67, 128, 129, 130, 193, 194, 195)
_alive_cache = {}


def alive_full(policy, window_len):
    key = (policy, window_len)
    if key not in _alive_cache:
        _alive_cache[key] = alive_stream(policy, window_len, max(ALIVE_NSEGS))
        _alive_cache[key].expected()
    return _alive_cache[key]


def alive_case(policy, window_len, nsegs, last_tokens=7):
    """the alive stream cut to nsegs segments, the last of them short (7 tokens)"""
    full = alive_full(policy, window_len)
    return full.prefix(nsegs, last_tokens, "alive/%s/w%d/nsegs%d" % (policy, window_len, nsegs))


@functools.lru_cache(maxsize=None)
def alignment_cases(policy="placed"):
    """(e): one 3-segment alive stream whose out_len ends 0 .. 15 bytes past a multiple of 16"""
    base = alive_case(policy, 0, 3)
    out = []
    for k in range(16):
        n = 3 + (k - base.out_len - 3) % 16
        s = base.extended([tok_match(n, CTX - k)], name="alive3/%s/end%d" % (policy, k))
        assert s.out_len % 16 == k
        out.append(s)
    return out


# ---- (f) windows --------------------------------------------------------------------------------------------------------
WINDOW_LENS = (0, 1, 257, 32767, 32768)


def window_streams(window_len, seed=0xF6):
    """small streams whose first token reaches the window's first byte, or is an overlapped copy out of the window"""
    out = []
    firsts = [(ln, window_len) for ln in (3, 258)] + [(ln, d) for d in (1, 2, 3, 64, 257) for ln in sorted({d + 1, 258})
                                                      if d <= window_len and 3 <= ln <= 258]
    if window_len == 0:
        firsts = [None]
    for k, first in enumerate(firsts):
        rng = np.random.default_rng(seed + 100 * k + window_len)
        window = rng.integers(0, 256, size=window_len, dtype=np.uint8).tobytes()
        b = _builder("decoder", window)
        if first is not None:
            b.match(*first)
            b.mark("first_len%d_dist%d" % first, 0)
        b.fill(rng, 37 + k)
        if window_len:
            at = b.out
            b.match(258, min(CTX, b.out + window_len))           # the window's first byte again, from further on
            b.match(200, min(CTX, b.out + window_len) - 1)
            b.mark("again", at)
        b.fill(rng, 11)
        out.append(b.finish("window%d/first%s" % (window_len, "_%d_%d" % first if first else "_literal")))
    return out


@functools.lru_cache(maxsize=None)
def window_alive(window_len):
    """130 segments; with a window the first segment is nothing but matches into it"""
    s = alive_stream("decoder", window_len, 130, seed=0xF7)
    return s.prefix(130, 7, "window_alive/w%d" % window_len)


# ---- (g) the batch layout -----------------------------------------------------------------------------------------------
def batch_streams(seed=0x67):
    """[(Stream, window bytes or None)] for one zng_rocm_inflate_many call; plaintext lengths 0, 1, 3, 32767, 32768, 32769,
    65536 + 5 and alive streams of 3, 40 and 30 segments; behind them one more of 3 and one of 70 segments"""
    rng = np.random.default_rng(seed)
    out = []

    def small(n, window_len, name):
        window = rng.integers(0, 256, size=window_len, dtype=np.uint8).tobytes()
        b = _builder("decoder", window)
        if window_len and n >= 3:
            b.match(min(n, 258), window_len)                     # the window's first byte
            b.mark("first", 0)
        while b.out < n:
            left = n - b.out
            if left >= 400 and b.out + window_len and rng.integers(0, 3) == 0:
                b.match(int(rng.integers(3, 259)), int(rng.integers(1, min(CTX, b.out + window_len) + 1)))
            else:
                b.fill(rng, min(left, int(rng.integers(1, 700))))
        assert b.out == n
        out.append(b.finish(name))

    small(0, 0, "batch/len0")
    small(1, 0, "batch/len1")
    small(3, 1, "batch/len3_w1")
    small(32767, 257, "batch/len32767_w257")
    small(32768, 32768, "batch/len32768_w32768")
    small(32769, 0, "batch/len32769")
    small(65536 + 5, 1, "batch/len65541_w1")
    out.append(alive_case("decoder", 32768, 3))
    out.append(alive_case("decoder", 0, 40))
    out.append(window_alive(257).prefix(30, 7, "batch/alive30_w257"))
    # which streams share a launch is the dispatcher's decision at run time; this one crosses a group border on its own
    out.append(window_alive(1).prefix(3, 7, "batch/alive3_w1"))
    out.append(window_alive(32767).prefix(70, 7, "batch/alive70_w32767"))
    return out


def fixed_stream(stream):
    """the token list as one fixed-Huffman block (tests/deflate_craft.py)"""
    import deflate_craft as craft
    bits = craft.Bits()
    craft.fixed_block(bits, stream.craft_tokens(), True)
    bits.align()
    return bytes(bits.out)


def k1_streams():
    """every crafted K1 stream: (a), (b) under both policies with and without a window, (c)"""
    out = [flush_mark_stream("decoder"), flush_mark_stream("placed")]
    for policy in ("decoder", "placed"):
        for wl in (0, CTX):
            out.append(previous_segment_stream(policy, wl))
        out.append(literal_window_stream(policy))
    return out + last_literals_streams()
