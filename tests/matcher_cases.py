"""Planted repeats for the two LZ77 match finders (test infrastructure; pure numpy, seeded): streams in which the bytes of one
range [at, at + m) have exactly ONE earlier copy, at a chosen distance D, and nothing else in the stream competes with it.
What a finder must then find is known without a model of the finder: the range is covered by matches of distance D.

A cell is (m, D, at, tail):
  far form   (D >= m)  zeros(at - D) + R + zeros(D - m) + R + zeros(tail); R = m random bytes in 1..255 whose m - 3 four-byte
                       strings are all distinct.  A zero run occupies one hash row / one head slot, so the filler cannot evict R
                       from any search structure (emitter_cases._dist_edges relies on the same fact).
  near form  (D < m)   zeros(at - D), a random unit of D bytes in 1..255 repeated to length m + D, zeros(tail); the D four-byte
                       strings of the repetition are all distinct, so the only earlier copies lie at multiples of D.
  dictionary form      the far form with the first R inside `dict_len` bytes of history in front of the stream.

coverage() walks a parsed token list with a running output position; budget_stream() builds the candidate-budget input.
The CPU tests (test_matcher_recall_cpu.py) hold the generators to these promises and CPython's zlib to the recall the GPU
tests (test_gpu_matcher_recall.py) ask of the device."""
import collections
import functools

import numpy as np

import deflate_parse as dp
from emitter_cases import BLOCK, SEGMENT

MAX_DIST = 32768 - 262                          # deflate.h:410-415, kLzMaxDist
REGION, BATCH_ROWS, BATCH_QUICK = 64, 1024, 256
BORDERS = (65 * REGION, 5 * BATCH_ROWS, BLOCK, SEGMENT)        # 4160, 5120 (20 quick batches as well), 61440, 131072

DISTANCES = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 32505, 32506)
TOO_FAR = (32507, 32768)
LENGTHS = (16, 17, 31, 32, 33, 63, 64, 65, 257, 258, 259, 262, 300, 520, 1024)
TAILS = (0, 1, 3, 257, 300, 600)
DICT_LENS = (300, 32506, 32768)
DICT_OFFS = (0, 5, 1023, 1024)


class Cell:
    """data: the stream; history: the dictionary in front of it (b"" for most); [at, at + m): the checked bytes of the
    stream; D: the distance of their one earlier copy; near: D < m; too_far: D > MAX_DIST, nothing may be found"""

    def __init__(self, sweep, m, D, at, tail, data, history=b""):
        self.sweep, self.m, self.D, self.at, self.tail = sweep, m, D, at, tail
        self.data, self.history = bytes(data), bytes(history)
        self.near, self.too_far = D < m, D > MAX_DIST
        self.name = "%s/m%d-D%d-at%d-tail%d%s" % (sweep, m, D, at, tail, "-dict%d" % len(history) if history else "")
        assert len(self.data) <= 165 << 10


def _grams(b):
    return [bytes(b[i:i + 4]) for i in range(len(b) - 3)]


def distinct_bytes(m, rng):
    """m random bytes in 1..255 whose m - 3 four-byte strings are all distinct"""
    while True:
        r = rng.integers(1, 256, size=m, dtype=np.uint8).tobytes()
        if len(set(_grams(r))) == max(m - 3, 0):
            return r


def unit_bytes(D, rng):
    """D random bytes in 1..255 whose repetition has D distinct four-byte strings (so its period is D and no less)"""
    while True:
        u = rng.integers(1, 256, size=D, dtype=np.uint8).tobytes()
        rep = (u * (4 // D + 2))[:D + 3]
        if len(set(_grams(rep))) == D:
            return u


def _seed(*key):
    return [0x4D41, *[int(k) for k in key]]


def planted(sweep, m, D, at, tail, salt=0):
    """one cell of the far or the near form"""
    assert at >= D >= 1 and m >= 4
    rng = np.random.default_rng(_seed(m, D, at, tail, salt))
    if D >= m:
        r = distinct_bytes(m, rng)
        data = bytes(at - D) + r + bytes(D - m) + r + bytes(tail)
    else:
        u = unit_bytes(D, rng)
        data = bytes(at - D) + (u * ((m + D) // D + 1))[:m + D] + bytes(tail)
    assert len(data) == at + m + tail
    return Cell(sweep, m, D, at, tail, data)


def planted_dict(m, dict_len, off, tail=300):
    """the dictionary form: R at the dictionary's first bytes -- or as far back as MAX_DIST allows --, again at stream
    offset `off`"""
    D = min(dict_len + off, MAX_DIST)
    src = dict_len + off - D
    assert D >= m and src + m <= dict_len
    rng = np.random.default_rng(_seed(m, dict_len, off, tail, 7))
    r = distinct_bytes(m, rng)
    history = bytes(src) + r + bytes(dict_len - src - m)
    return Cell("dict", m, D, off, tail, bytes(off) + r + bytes(tail), history)


@functools.lru_cache(maxsize=None)
def cells():
    out = []
    for m in (16, 64, 300):                                                    # distance sweep
        out += [planted("dist", m, D, 40000, 300) for D in DISTANCES + TOO_FAR]
    for m in (16, 258, 300):                                                   # position sweep
        for D in (1, 7, 1500, MAX_DIST):
            if D == 1 and m == 258:
                continue
            for b in BORDERS:
                for at in (b - 1, b, b + 1) + ((b - 130,) if m >= 258 else ()):
                    if at >= D:
                        out.append(planted("pos", m, D, at, 300))
    for m in LENGTHS:                                                          # length sweep
        out += [planted("len", m, D, 40000, 300, salt=1) for D in (3, 4096)]
    for tail in TAILS:                                                         # tail sweep
        out += [planted("tail", m, D, 40000, tail, salt=2) for m in (16, 300) for D in (7, 4096)]
    for dict_len in DICT_LENS:                                                 # dictionary cells
        out += [planted_dict(m, dict_len, off) for off in DICT_OFFS for m in (16, 300)]
    assert len({c.name for c in out}) == len(out)
    return out


def segment_border(c):
    """the 131072 border inside (at, at + m), or None: the rows class ends every match at its segment's end"""
    return SEGMENT if not c.history and c.at < SEGMENT < c.at + c.m else None


Cover = collections.namedtuple("Cover", "lits dists max_dist min_reach ntokens")


def coverage(parsed, lo, hi, hist_len=0):
    """Cover of the parsed stream for the byte range [lo, hi): how many of its bytes are literals (bytes of stored blocks
    included), the distances of the match tokens that overlap it, the largest distance of any token of the stream, the
    lowest position any token copies from (counted from the first byte of the history) and the number of tokens that
    overlap the range"""
    lits, dists, max_dist, min_reach, ntok = 0, set(), 0, hist_len, 0

    def literal_run(a, b):
        nonlocal lits, ntok
        k = min(b, hi) - max(a, lo)
        if k > 0:
            lits += k
            ntok += k

    for b in parsed.blocks:
        if b.btype == dp.STORED:
            literal_run(b.out_start, b.out_end)
            continue
        pos, prev = b.out_start, -1
        for i, length, dist, _ in b.matches:
            literal_run(pos, pos + i - prev - 1)
            pos += i - prev - 1
            if pos < hi and pos + length > lo:
                dists.add(dist)
                ntok += 1
            max_dist = max(max_dist, dist)
            min_reach = min(min_reach, pos + hist_len - dist)
            pos += length
            prev = i
        rest = len(b.lit_syms) - 1 - prev - 1                                  # literals behind the last match; not the end-of-block
        literal_run(pos, pos + rest)
        assert pos + rest == b.out_end
    return Cover(lits, dists, max_dist, min_reach, ntok)


# ---- the candidate budget ---------------------------------------------------------------------------------------------------
GAP = 1100                                      # zeros between two strings: more than a 1024-position batch
BUDGET_T = 200


class BudgetStream:
    """data; query: where X + T stands the second time; dist: the distance of the true source; k, rot"""


def budget_stream(k, rot, seed=0):
    """A true source X + T, k decoys X + random_i (12 bytes each), the query X + T, everything separated by at least GAP
    zeros: when the query is searched, k + 1 candidates with its first four bytes lie in front of its batch.  In front of
    them, more than MAX_DIST before the query and so no candidates of it, stand `rot` more strings X + random: a finder that
    keeps a fixed number of recent positions per hash then holds the true source in another slot for every rot, whatever
    the order in which it looks at them.  Whatever that order, a finder whose budget is at least k + 1 sees the true
    source."""
    rng = np.random.default_rng(_seed(k, rot, seed, 11))
    while True:
        x = rng.integers(1, 256, size=4, dtype=np.uint8).tobytes()
        t = rng.integers(1, 256, size=BUDGET_T, dtype=np.uint8).tobytes()
        others = [x + rng.integers(1, 256, size=8, dtype=np.uint8).tobytes() for _ in range(rot + k)]
        grams = _grams(x + t) + [g for o in others for g in _grams(o)[1:]]
        if len(set(grams)) == len(grams) and all(o[4] != t[0] for o in others):
            break
    s = BudgetStream()
    data = bytearray(GAP)
    for o in others[:rot]:
        data += o + bytes(GAP)
    data += bytes(MAX_DIST + 500)
    true_at = len(data)
    data += x + t + bytes(GAP)
    for o in others[rot:]:
        data += o + bytes(GAP)
    s.query = len(data)
    data += x + t + bytes(300)
    s.data, s.dist, s.k, s.rot, s.x, s.t = bytes(data), s.query - true_at, k, rot, x, t
    s.decoys = others[rot:]
    s.name = "budget/k%d-rot%d" % (k, rot)
    assert s.dist <= MAX_DIST and len(s.data) < SEGMENT
    return s


@functools.lru_cache(maxsize=None)
def budget_streams():
    return [budget_stream(k, rot) for k in (0, 1, 2, 5, 7) for rot in range(8)]


def pack(items):
    """the existing tests' layout: every history + stream at a 16-byte aligned offset, 16 readable bytes behind the last.
    items: (history, data) -> (host array, stream offsets, stream lengths, history lengths)"""
    offs, lens, dls, pos = [], [], [], 0
    for history, data in items:
        pos += -(pos + len(history)) % 16                                      # the STREAM starts aligned, its history before it
        offs.append(pos + len(history))
        lens.append(len(data))
        dls.append(len(history))
        pos += len(history) + len(data)
        pos += -pos % 16
    host = np.zeros(pos + 16, dtype=np.uint8)
    for (history, data), o in zip(items, offs):
        both = history + data
        host[o - len(history):o - len(history) + len(both)] = np.frombuffer(both, dtype=np.uint8)
    return host, offs, lens, dls
