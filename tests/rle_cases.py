"""Crafted runs for the Z_RLE / Z_HUFFMAN_ONLY front end (rle_rows_kernel, deflate_rle.h; test infrastructure, pure numpy,
seeded): streams in which one run of equal bytes is placed, to the byte, against one border of the kernel's mapping -- a lane, a
wave, a 4096-position batch, a 61440-position block, a 131072-byte segment, the end of the history -- inside noise in which
every position is a break.  What the kernel must then write is known from the greedy parse of deflate_rle.c alone
(strategy_util.rle_parse, which tests/test_deflate_strategy_cpu.py pins to CPython's own Z_RLE tokens).

All positions count from the first history byte, as the kernel counts them.  A stream's segment i is [a, b) with
a = dict_len + i * SEGMENT; its first batch begins at first = a - a % ALIGN, its batch borders are P = first + k * BATCH and
its blocks end at first + k * BLOCK.

A case: name, family, history (bytes in front, possibly empty), data, and edge -- {"kind": ..., parameters}: the property it was
built for, which tests/test_rle_cases_cpu.py derives again from the model's token starts and breaks (a case that does not
reach its edge fails there).  The kinds:
  carry      a run [s, s + L) holds no break on `borders` batch borders: those batches take their chain origin from carry_o
  nocarry    a run of about one batch that ends 0 or 1 positions in front of the border: nothing may be carried over it
  tail       a run that ends at `end` = border + d with the last chain point at `point` = end - r and r bytes left
  ahead      a chain point at `point` = P - k, k <= 258, whose run ends at `end` >= P: the length comes from the read-ahead
             (`match`: the run is 3 or longer; `limit`: what stops the read-ahead -- "byte", "stream" or "segment")
  segment    a run over the segment border `border` that leaves r bytes of its 258-chain in front and t bytes behind
  length     a stream of SEGMENT + t bytes: a last segment of t bytes
  block      a run over the block border `border`; `point`: a chain point placed on it (None: wherever the chain puts one)
  history    the stream starts at a = dict_len; `cont`: it continues the history's last run, which is `run` long
  plain      nothing placed"""
import functools
import zlib

import numpy as np

import strategy_util as su
from emitter_cases import BLOCK, SEGMENT       # 61440 (kSubBytes), 131072 (kSegBytesMin): deflate_rows_plan.h:42, :26

BATCH = 4096                                    # kRleBatch, deflate_rle.h:34
LANE = 16                                       # kRlePer, deflate_rle.h:33
WAVE = 1024                                     # 64 lanes (deflate_rle.h:52) of kRlePer positions
ALIGN = 1024                                    # kRowsBatch, deflate_rows_plan.h:24 (kRowBatch at deflate_rle.h:53)
CHAIN = 258                                     # the longest match: the period of the chain (deflate_rle.h:145)
HIST_MAX = 32768                                # kPrime, deflate_rows_plan.h:35: the most a dict_len may be

NOISE = tuple(range(0x60, 0x68))                # noise bytes; the placed runs use RUN, the filler's own runs FILL
RUN = (0x01, 0x02)
FILL = tuple(range(0x70, 0x74))

FAMILIES = ("long", "tail", "ahead", "segment", "block", "history", "plain")
LONG_L = (4095, 4096, 4097, 16 * CHAIN, 16 * CHAIN + 1, 16 * CHAIN + 2, 16 * CHAIN + 3, 2 * BATCH + 257, BLOCK + 5)
LONG_S = (0, 1, 2, 15, 16, 17, 1023, 4095)
TAIL_D = (-3, -2, -1, 0, 1, 2, 3)
TAIL_BORDERS = (("batch", BATCH), ("wave", BATCH + WAVE), ("lane", BATCH + LANE))
AHEAD_K = (1, 2, 3, 15, 16, 17, 257, 258)
AHEAD_E = (0, 1, 15, 16, 17, 31, 32, 33)
SEG_R = (0, 1, 2, 3)
SEG_T = (0, 1, 2, 3, 4, 300)
HIST_LENS = (1, 5, 1023, 1024, 1025, 4095, 4097, 32768)
HIST_RUNS = (1, 3, 258, 700)


class Case:
    def __init__(self, name, data, history=b"", **edge):
        self.name, self.family = name, name.split("/")[0]
        self.data, self.history, self.edge = bytes(data), bytes(history), edge
        assert self.family in FAMILIES and "kind" in edge
        assert len(self.data) < 3 * SEGMENT + 4096 and len(self.history) <= HIST_MAX

    @property
    def dict_len(self):
        return len(self.history)


def noise(n, *key):
    """n bytes of NOISE in which no two neighbours are equal: every position is a break"""
    rng = np.random.default_rng([0x524C45] + [int(k) for k in key])
    steps = rng.integers(1, len(NOISE), size=n)
    return (NOISE[0] + np.cumsum(steps) % len(NOISE)).astype(np.uint8).tobytes()


def run(n, value=RUN[0]):
    return bytes([value]) * n


def filler(n, *key):
    """n bytes for the long stretches in front of a far border: noise and runs of FILL bytes in turn -- tokens of every kind
    for the blocks' histograms, and fewer of them than noise alone would make"""
    rng = np.random.default_rng([0x46494C] + [int(k) for k in key])
    parts, size, k = [], 0, 0
    while size < n:
        m = int(rng.integers(20, 400)) if k % 2 == 0 else int(rng.integers(1, 3000))
        parts.append(noise(m, size, *key) if k % 2 == 0 else run(m, FILL[int(rng.integers(0, len(FILL)))]))
        size += m
        k += 1
    return b"".join(parts)[:n]


def _key(name):
    return zlib.crc32(name.encode())


def _long():
    out = []
    for L in LONG_L:
        for s in LONG_S:
            name = "long/L%d-s%d" % (L, s)
            borders = [P for P in range(BATCH, s + L, BATCH) if s < P]          # P - 1 and P both inside the run
            edge = dict(kind="carry", borders=len(borders)) if borders else dict(kind="nocarry")
            out.append(Case(name, noise(s, _key(name)) + run(L) + noise(40, _key(name), 1), start=s, length=L, **edge))
    return out


def _tail():
    """a run of 1 + 258 m + r bytes (its first byte is a break, the chain behind it leaves r) that ends at border + d"""
    out = []
    for which, B in TAIL_BORDERS:
        for d in TAIL_D:
            for m, r in [(0, 1), (0, 2), (0, 3)] + [(1, r) for r in (0, 1, 2, 3)]:
                name = "tail/%s%+d-m%d-r%d" % (which, d, m, r)
                L, end = 1 + CHAIN * m + r, B + d
                s = end - L
                data = noise(s, _key(name)) + run(L) + noise(BATCH + 2 * WAVE - end, _key(name), 1)
                out.append(Case(name, data, kind="tail", border=B, which=which, end=end, point=end - r, r=r, start=s))
    return out


def _ahead():
    out = []
    for P, limit in ((BATCH, "byte"), (BATCH, "stream")):
        for k in AHEAD_K:
            for e in AHEAD_E + (CHAIN - k,):
                if k + e > CHAIN or (e == CHAIN - k and e in AHEAD_E):   # the run ends within the chain point's match
                    continue
                name = "ahead/k%d-e%d-%s" % (k, e, limit)
                c = P - k                                                       # the chain point; the run's first byte before it
                data = noise(c - 1, _key(name)) + run(1 + k + e) + (noise(300, _key(name), 1) if limit == "byte" else b"")
                out.append(Case(name, data, kind="ahead", border=P, point=c, end=P + e, match=k + e >= 3, limit=limit))
    for k in (1, 3, 17, 258):                   # the segment ends on the batch border: the run goes on, the match does not
        name = "ahead/k%d-segment" % k
        c = SEGMENT - k
        data = filler(c - 1, _key(name)) + run(1 + k + 40) + noise(300, _key(name), 1)
        out.append(Case(name, data, kind="ahead", border=SEGMENT, point=c, end=SEGMENT, match=k >= 3, limit="segment"))
    return out


def _segment():
    out = []
    for r in SEG_R:
        for t in SEG_T:
            name = "segment/r%d-t%d" % (r, t)
            s = SEGMENT - r - 2 * CHAIN - 1                                      # break at s, chain points at s + 1 + 258 k
            data = filler(s, _key(name)) + run(SEGMENT + t - s) + noise(500, _key(name), 1)
            out.append(Case(name, data, kind="segment", border=SEGMENT, r=r, t=t, start=s))
    for t in (0, 1, 2, 3):
        for tag, tailb in (("run", run(8 + t)), ("noise", noise(8 + t, t))):
            name = "segment/len+%d-%s" % (t, tag)
            out.append(Case(name, filler(SEGMENT - 8, _key(name)) + tailb, kind="length", t=t))
    out.append(Case("segment/run2seg+7", run(2 * SEGMENT + 7), kind="segment", border=SEGMENT, r=(SEGMENT - 1) % CHAIN, t=SEGMENT + 7,
                    start=0))
    return out


def _block():
    out = []
    lead = lambda n, name: filler(n, _key(name))
    out.append(Case("block/across300", lead(BLOCK - 300, "b0") + run(600) + noise(300, 1), kind="block", border=BLOCK, point=None))
    for d in (-1, 0, 1):                        # a 258-match ends, and the next chain point stands, on border + d
        name = "block/point%+d" % d
        s = BLOCK + d - CHAIN - 1
        out.append(Case(name, lead(s, name) + run(1 + CHAIN + 100) + noise(300, 2 + d), kind="block", border=BLOCK, point=BLOCK + d))
    # the stream ends inside the match that runs over the border: the last block, [BLOCK, BLOCK + 50), has no token of its own
    out.append(Case("block/empty_last", lead(BLOCK - 101, "b1") + run(151), kind="block", border=BLOCK, point=None))
    # the same border inside the second segment (its blocks count from its own first batch) with 5 bytes of history: first < a
    name = "block/second_segment"
    border = 5 + SEGMENT - (5 + SEGMENT) % ALIGN + BLOCK
    out.append(Case(name, lead(border - 300 - 5, name) + run(600) + noise(300, 7), history=noise(5, 8), kind="block",
                    border=border, point=None))
    return out


def _history():
    out = []
    for dl in HIST_LENS:
        for hr in HIST_RUNS:
            for cont in (False, True):
                name = "history/d%d-run%d-%s" % (dl, hr, "cont" if cont else "noise")
                hist = (noise(max(dl - hr, 0), _key(name)) + run(hr))[-dl:]
                data = (run(600) if cont else b"") + noise(BATCH + 700, _key(name), 1) + run(300, RUN[1]) + noise(100, _key(name), 2)
                out.append(Case(name, data, history=hist, kind="history", cont=cont, run=min(hr, dl)))
    for ph in range(LANE):                      # first < a, with a at each phase within a lane
        dl = 2 * ALIGN + 3 * LANE + ph
        name = "history/phase%d" % ph
        hist = noise(dl - 258, _key(name)) + run(258)
        data = run(2 * CHAIN + 3 + ph) + noise(BATCH, _key(name), 1)
        out.append(Case(name, data, history=hist, kind="history", cont=True, run=258))
    for dl in (HIST_MAX, 4097):                 # the second segment starts in a run too: a = dl + SEGMENT, its own first < a
        name = "history/d%d-two-segments" % dl
        hist = noise(dl - 700, _key(name)) + run(700)
        s = SEGMENT - 400
        data = run(300) + filler(s - 300, _key(name)) + run(700, RUN[1]) + noise(SEGMENT + 300 - s - 700, _key(name), 1)
        out.append(Case(name, data, history=hist, kind="history", cont=True, run=700))
    return out


def _plain():
    out = [Case("plain/n%d" % n, run(n, 0x7a), kind="plain") for n in range(5)]
    out += [Case("plain/run_heavy%d" % s, su.run_heavy(SEGMENT + 5000, seed=s), kind="plain") for s in (61, 62)]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = _long() + _tail() + _ahead() + _segment() + _block() + _history() + _plain()
    assert len({c.name for c in out}) == len(out)
    assert sum(len(c.history) + len(c.data) + 32 for c in out) < 32 << 20      # one batched call still cuts SEGMENT-byte segments
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)


def family(name):
    return [c for c in cases() if c.family == name]


def segments(case):
    """[(a, b)]: the segments of the stream, in positions; an empty stream is one empty segment"""
    d, n = case.dict_len, len(case.data)
    return [(d + i, min(d + i + SEGMENT, d + n)) for i in range(0, max(n, 1), SEGMENT)]


def block_ranges(case):
    """[(lo, hi)]: the blocks the plan cuts (deflate_rows_plan.h:246-259), per segment [max(a, first + k BLOCK), min(b, first +
    (k + 1) BLOCK)); the one block of an empty stream is empty"""
    out = []
    for a, b in segments(case):
        first = a - a % ALIGN
        nsub = -(-(b - first) // BLOCK) if b > first else 1
        out += [(max(a, first + k * BLOCK), min(b, first + (k + 1) * BLOCK)) for k in range(nsub)]
    return out


def batch_borders(case):
    """every batch border P = first + k * BATCH, k >= 1, below its segment's end"""
    return [P for a, b in segments(case) for P in range(a - a % ALIGN + BATCH, b, BATCH)]


def stream_tokens(history, data):
    """the tokens of one stream behind `history` (not a case of the list: the hook's blocks)"""
    c = Case("plain/-", data, history, kind="plain")
    return [t for a, b in segments(c) for t in su.rle_parse(c.history + c.data, a, b)]


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = by_name(name)
    both = c.history + c.data
    return tuple(tuple(su.rle_parse(both, a, b)) for a, b in segments(c))


def expected_tokens(case):
    """the tokens the device must write: the greedy parse of deflate_rle.c, independently per segment"""
    return [t for seg in _expected(case.name) for t in seg]


def token_starts(case):
    """[(position, token)] of expected_tokens"""
    out = []
    for (a, _), toks in zip(segments(case), _expected(case.name)):
        p = a
        for t in toks:
            out.append((p, t))
            p += t[1] if t[0] == 'm' else 1
    return out


def breaks(case):
    """bool per position of history + data: the byte differs from the one before it (position 0 is a break)"""
    d = np.frombuffer(case.history + case.data, dtype=np.uint8)
    return np.concatenate(([True], d[1:] != d[:-1])) if d.size else np.zeros(0, dtype=bool)
