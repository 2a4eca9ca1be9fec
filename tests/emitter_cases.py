"""Crafted inputs for the block emitter (emit_dynamic_kernel; test infrastructure): plaintexts whose block histograms are
chosen, not met by accident.  Z_HUFFMAN_ONLY makes every input byte one literal, so a block's literal histogram is the byte
histogram of its 61440 positions (plus one end-of-block) -- the handle of most cases.  Everything is seeded and deterministic;
every case carries the condition it was built for, which the CPU tests assert on the generator's own histogram and on
CPython's block, and the GPU tests on the product's parsed block.

A case: name, data, strategy, level, and what it was built for:
  hist      the literal/length histogram the generator intends, end-of-block included (literal-only cases)
  deep      {"lit" | "dist" | "cl": limit}  that code set's histogram has min_max_depth > limit in SOME block
  exact     {"lit" | "cl": limit}           ... has min_max_depth == limit in its one block
  cl_hist   the code-length-symbol histogram the generator intends (cl cases)
  single    the case is one block for CPython at memLevel 9 (<= 32767 bytes): its block is the cost reference
  extra     whatever else a family knows of its cases (lit_lens: the only optimal lengths; k, n; alphabets; the sizes and
            the block type dyn_tie predicts)"""
import functools

import numpy as np

Z_DEFAULT_STRATEGY, Z_HUFFMAN_ONLY, Z_RLE, Z_FIXED = 0, 2, 3, 4
BLOCK = 61440                                   # positions per block of a segment
SEGMENT = 128 << 10                             # plaintext per segment for inputs of this size


class Case:
    def __init__(self, name, data, strategy=Z_HUFFMAN_ONLY, level=6, **pre):
        self.name, self.data, self.strategy, self.level = name, bytes(data), strategy, level
        self.deep, self.exact = pre.pop("deep", {}), pre.pop("exact", {})
        self.cl_hist, self.single = pre.pop("cl_hist", None), pre.pop("single", False)
        self.hist = pre.pop("hist", None)
        self.extra = pre
        assert len(self.data) <= 256 << 10 and (not self.single or len(self.data) <= 32767)


def series(k):
    """a(n) = a(n-1) + a(n-2) + 1: 1, 1, 3, 5, 9, 15, ... -- no two partial sums tie, so the Huffman tree of the first k
    terms is a chain whichever way ties would be broken"""
    a = [1, 1]
    while len(a) < k:
        a.append(a[-1] + a[-2] + 1)
    return a[:k]


def _shuffled(counts, seed):
    """counts: {byte value: how often} -> the bytes in random order"""
    vals = np.repeat(np.array(list(counts), dtype=np.uint8), list(counts.values()))
    np.random.default_rng(seed).shuffle(vals)
    return vals.tobytes()


def _lit_hist(counts):
    h = [0] * 286
    for v, c in counts.items():
        h[v] = c
    h[256] = 1
    return h


def _series_case(name, k, seed, pad_to=0, scale=1, **pre):
    """scale: every count so many times -- a power of two of them survives that many halvings of all frequencies unchanged"""
    vals = [(37 * i + 11) % 256 for i in range(k)]           # k distinct byte values on both sides of 144
    counts = dict(zip(vals, [scale * a for a in series(k)]))
    if pad_to:
        counts[vals[-1]] += pad_to - sum(counts.values())
    return Case(name, _shuffled(counts, seed), hist=_lit_hist(counts), **pre)


def _dyadic(lens_by_byte, lmax, seed):
    """byte value v 2^(lmax - L_v) times; with the end-of-block (once, so L = lmax) the counts are exact powers of two of a
    full code, and the optimal lengths are exactly L_v"""
    counts = {v: 1 << (lmax - n) for v, n in lens_by_byte.items()}
    assert sum(counts.values()) + 1 == 1 << lmax, "the lengths (end-of-block included) must be a complete code"
    return counts, _shuffled(counts, seed)


def _cl_case(name, multiset, zeros, long_run, **pre):
    """the code-length tree: `multiset` {length: how many symbols, end-of-block included}, `zeros` single zero lengths and
    one zero run of `long_run` between the used byte values, no four equal lengths side by side (no repeat code), the forced
    distance lengths 1, 1 behind: the code-length symbols then count multiset + {0: zeros, 18: 1, 1: 2}"""
    lmax = max(multiset)
    syms = [n for n, c in sorted(multiset.items()) for _ in range(c)]
    syms.remove(lmax)                                        # the end-of-block's
    assert len(syms) + zeros + long_run == 256 and 11 <= long_run <= 138
    for seed in range(1000):
        rng = np.random.default_rng(seed)
        order = [syms[i] for i in rng.permutation(len(syms))]
        big = int(rng.integers(0, len(order) - 1))           # the junction (behind order[big]) of the long run
        gaps, run = set(), 1
        for i in range(1, len(order) + 1):
            nxt = order[i] if i < len(order) else lmax       # (the end-of-block follows the last one)
            if i - 1 == big or order[i - 1] != nxt:
                run = 1
            elif run == 3:
                gaps.add(i - 1)
                run = 1
            else:
                run += 1
        free = [j for j in range(len(order) - 1) if j != big and j not in gaps]
        if len(gaps) > zeros or len(free) < zeros - len(gaps):
            continue
        gaps |= set(int(j) for j in rng.choice(free, size=zeros - len(gaps), replace=False))
        lens, v = {}, 0
        for i, n in enumerate(order):
            lens[v] = n
            v += 1 + (1 if i in gaps else 0) + (long_run if i == big else 0)
        assert v == 256
        counts, data = _dyadic(lens, lmax, seed)
        cl = dict(multiset)
        cl[0], cl[18], cl[1] = zeros, 1, cl.get(1, 0) + 2
        return Case(name, data, hist=_lit_hist(counts), cl_hist=[cl.get(s, 0) for s in range(19)], single=True, **pre)
    raise AssertionError("no arrangement found")


def _rle_header_cases():
    """length sequences that drive every path of the code-length run coder.  a: zero runs of 2, 3, 10, 11 and 138 between
    equal non-zero lengths in runs of 3, 4, 7, 8 and 13, a run of 5, and 47 zeros that end at byte 255 with the end-of-block
    behind them; b / c: zero runs of 139 (138 + a single zero) and 149 (138 + 11) in a chain of lengths 1 .. 12"""
    seq = [3] * 3 + [0] * 2 + [4] * 4 + [0] * 3 + [6] * 7 + [0] * 10 + [6] * 8 + [0] * 11 + [8] * 13 + [0] * 138 + \
          [6] * 5 + [8] * 2 + [10] * 3
    seq += [0] * (256 - len(seq))
    out = []
    counts, data = _dyadic({v: n for v, n in enumerate(seq) if n}, 10, 70)
    out.append(Case("rle_header/a", data, hist=_lit_hist(counts), single=True, lit_lens=seq + [10]))
    for tag, gap in (("b", 139), ("c", 149)):
        seq = [1, 2, 3, 4, 5, 6] + [0] * gap + [7, 8, 9, 10, 11, 12]
        seq += [0] * (256 - len(seq))
        counts, data = _dyadic({v: n for v, n in enumerate(seq) if n}, 12, 71)
        out.append(Case("rle_header/" + tag, data, hist=_lit_hist(counts), single=True, lit_lens=seq + [12]))
    # one byte value and the end-of-block, one bit each, next to the two forced distance lengths of one bit: a run of equal
    # lengths from the literal/length lengths into the distance lengths
    out.append(Case("rle_header/cross", b"x" * 3000, hist=_lit_hist({ord("x"): 3000}), single=True,
                    lit_lens=[1 if v in (ord("x"), 256) else 0 for v in range(257)]))
    return out


def _blocks_differ():
    """200 KiB: the consecutive 61440-byte blocks of a segment draw from disjoint byte alphabets with different skews"""
    rng = np.random.default_rng(90)
    n = 200 << 10
    out = np.zeros(n, dtype=np.uint8)
    alphabets = []
    bounds = []
    for seg in range(0, n, SEGMENT):
        for lo in range(seg, min(seg + SEGMENT, n), BLOCK):
            bounds.append((lo, min(lo + BLOCK, seg + SEGMENT, n)))
    for k, (lo, hi) in enumerate(bounds):
        base, width = 64 * ((k + k // 3) % 4), (64, 40, 17, 64, 29)[k % 5]
        p = np.array([(0.5, 0.9, 0.75, 0.97, 0.8)[k % 5] ** i for i in range(width)])
        out[lo:hi] = base + rng.choice(width, size=hi - lo, p=p / p.sum())
        alphabets.append((lo, hi, base, base + width))
    return Case("blocks_differ", out.tobytes(), alphabets=alphabets)


def fixed_tie(k, n=100):
    """n distinct bytes in random order (no match), exactly k of them >= 144 (nine static bits instead of eight): the static
    block is ceil((3 + 7 + 8 n + k) / 8) bytes, the stored one n + 5"""
    rng = np.random.default_rng(1000 + k)
    vals = np.concatenate([rng.permutation(144)[:n - k], 144 + rng.permutation(112)[:k]]).astype(np.uint8)
    rng.shuffle(vals)
    return Case("fixed_tie/%d" % k, vals.tobytes(), strategy=Z_FIXED, k=k, n=n)


def predicted_header_bits(lit_lens, dist_lens):
    """the dynamic header of these lengths, first block bit to last code length, where the lengths leave no choice: the
    greedy run coding every encoder uses (deflate_craft.rle), HCLEN from the symbols it needs, and a code-length code of
    optimal cost -- unique as long as its tree stays within 7 bits"""
    import deflate_craft as craft
    import huffman_model as hm
    hist = [0] * 19
    extra = 0
    for s in craft.rle(list(lit_lens) + list(dist_lens), "greedy"):
        hist[s[0] if isinstance(s, tuple) else s] += 1
        extra += {16: 2, 17: 3, 18: 7}[s[0]] if isinstance(s, tuple) else 0
    assert hm.min_max_depth(hist) <= 7
    hclen = max([4] + [k + 1 for k in range(19) if hist[craft.CL_ORDER[k]]])
    return 3 + 5 + 5 + 4 + 3 * hclen + hm.optimal_cost(hist) + extra


TIE_GAPS = 10


def dyn_tie(high, gaps=TIE_GAPS):
    """255 bytes of 129 values: 126 of them twice, three once -- with the end-of-block exact powers of two of a full code, so
    seven and eight bits and no other optimal lengths.  `high` of the values that occur twice are >= 144 (one more static bit
    per byte); the first `gaps` values and the high ones stand alone between unused ones (each makes the dynamic header
    longer).  The static size grows with `high` faster than the dynamic one, and both are known here without running anything
    (extra: dyn_lenb, static_lenb, stored_lenb, btype)."""
    import huffman_model as hm
    low = 129 - high
    vals = [2 * i for i in range(gaps)] + list(range(2 * gaps, low + gaps)) + list(range(144, 144 + 3 * high, 3))
    assert len(set(vals)) == 129 and vals[low - 1] < 144
    lens = [0] * 257
    for i, v in enumerate(vals):
        lens[v] = 8 if low - 3 <= i < low else 7
    lens[256] = 8
    counts, data = _dyadic({v: n for v, n in enumerate(lens[:256]) if n}, 8, 2000 + high)
    hist = _lit_hist(counts)
    dyn = hm.dyn_lenb(predicted_header_bits(lens, [1, 1]), hist, [0] * 30, lens, [1, 1])
    static, stored = hm.static_lenb(hist, [0] * 30), hm.stored_lenb(len(data))
    btype = 0 if stored <= min(static, dyn) else (1 if static <= dyn else 2)
    return Case("dyn_tie/%d" % high, data, hist=hist, lit_lens=lens, dyn_lenb=dyn, static_lenb=static, stored_lenb=stored,
                btype=btype, single=True)


def stored_tie(k):
    """fixed_tie's bytes under Z_HUFFMAN_ONLY: the same tie between stored and static where all three block types compete
    (a dynamic block of 100 scattered symbols is far larger than either)"""
    c = fixed_tie(k)
    return Case("stored_tie/%d" % k, c.data, strategy=Z_HUFFMAN_ONLY, k=k, n=c.extra["n"])


DIST_CODES = list(range(28, 11, -1))            # dist_deep: code 28 is met once, code 12 most often
_DIST_LO = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
            8193, 12289, 16385, 24577, 32769)   # RFC 1951 3.2.5: the first distance of every code


def _dist_deep():
    """the distance tree: one block of 61440 random bytes (stored), then one block of 6-byte copies out of the 32 KiB before
    them, one fresh random byte between two copies; the copies' distance codes follow series(17) over the codes 28 .. 12.
    A copy's six bytes occur once in its window, so the matcher has one place to take them from -- where it finds it."""
    rng = np.random.default_rng(0xD157)
    want = dict(zip(DIST_CODES, series(len(DIST_CODES))))
    units = np.repeat(np.array(list(want)), list(want.values()))
    rng.shuffle(units)
    fill = BLOCK - 7 * units.size
    data = bytearray(rng.integers(0, 256, size=BLOCK + fill // 2, dtype=np.uint8).tobytes())
    fresh = rng.integers(0, 256, size=units.size, dtype=np.uint8).tolist()
    for code, sep in zip(units.tolist(), fresh):
        p = len(data)
        lo, hi = _DIST_LO[code], min(_DIST_LO[code + 1], _DIST_LO[code] + 512)      # the near end of the code's distances
        for _ in range(64):
            d = int(rng.integers(lo, hi))
            s = bytes(data[p - d:p - d + 6])
            if data.count(s, p - 32768 - 6, p) == 1:
                break
        else:
            raise AssertionError("no unique source")
        data += s
        data.append(sep)
    data += rng.integers(0, 256, size=2 * BLOCK - len(data), dtype=np.uint8).tobytes()
    hist = [0] * 30
    for c, f in want.items():
        hist[c] = f
    return Case("dist_deep", data, strategy=Z_DEFAULT_STRATEGY, dist_hist=hist, deep={"dist": 15})


def _dist_edges():
    rng = np.random.default_rng(0xED6E)
    # every match at distance 40 (code 10): 40 fresh random bytes, twice.  Byte values of nine static bits, so that a dynamic
    # block pays; no four bytes occur twice but in a unit's two halves, so that the matcher has no other distance to find
    one = b"".join(2 * rng.integers(144, 256, size=40, dtype=np.uint8).tobytes() for _ in range(100))
    where = {}
    for i in range(len(one) - 3):
        where.setdefault(one[i:i + 4], []).append(i)
    assert all(len(w) == 1 or (len(w) == 2 and w[1] - w[0] == 40) for w in where.values())
    # distance 1 (code 0) and a distance above 24576 (code 29) in one block: 64 random bytes, a run of one byte value that
    # leaves the search structure's other rows alone, the same 64 bytes again
    x = rng.integers(1, 17, size=64, dtype=np.uint8).tobytes()
    far = x + bytes(26000) + x + b"the end"
    return [Case("dist_one", one, strategy=Z_DEFAULT_STRATEGY),
            Case("dist_all", far, strategy=Z_DEFAULT_STRATEGY),
            Case("len_258", b"q" * 50000 + b"r" * 7000, strategy=Z_RLE)]


def mixed():
    """64 KiB of noise, 64 KiB of text, 64 KiB of the lit_deep bytes: every block type in one stream"""
    import synth
    rng = np.random.default_rng(0x313)
    deep = _series_case("x", 21, 13, pad_to=64 << 10).data
    return rng.integers(0, 256, size=64 << 10, dtype=np.uint8).tobytes() + synth.silesia_like(64 << 10, seed=77).tobytes() + deep


@functools.lru_cache(maxsize=None)
def cases():
    out = [
        _series_case("lit_deep", 18, 11, deep={"lit": 15}, single=True),
        _series_case("lit_deep/block", 18, 12, pad_to=BLOCK, scale=4, deep={"lit": 15}),
        _series_case("lit_exact15", 15, 13, exact={"lit": 15}, single=True),
        _cl_case("cl_deep", {3: 1, 4: 6, 5: 10, 6: 4, 8: 17, 10: 27, 11: 66}, 80, 46, deep={"cl": 7}),
        _cl_case("cl_exact7", {3: 1, 4: 4, 5: 7, 6: 11, 7: 15, 8: 17, 9: 26}, 38, 138, exact={"cl": 7}),
        _dist_deep(),
    ]
    out += _dist_edges() + _rle_header_cases() + [_blocks_differ()]
    out += [fixed_tie(k) for k in range(20, 34)] + [stored_tie(k) for k in range(20, 34)] + [dyn_tie(h) for h in range(0, 12)]
    out += [Case("mixed/default", mixed(), strategy=Z_DEFAULT_STRATEGY), Case("mixed/huffman", mixed())]
    assert len({c.name for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in cases() if c.name == name)
