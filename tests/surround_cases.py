"""Device deflate inputs at every alignment, in surroundings built to be mistaken for input (test infrastructure; plain Python
and numpy, seeded, no GPU).  include/zng_rocm.h promises every device deflate call an input at ANY alignment with `dict_len`
bytes of history directly in front of it, and nothing about the bytes behind the input or in front of the history.  The cases
here put bytes there that a guard which is off by one would take:

  case      (history H, plaintext P, front bait F, tail bait T); F and T are functions of H and P alone
  tail      P ends inside a repeat of distance D: P[-k:] == P[-k-D:-D] with k >= 8, and T is what continues that repeat,
            T[j] == (P + T)[len(P) + j - D] for BAIT = 600 bytes (more than two 258-byte matches).  D = 1: P ends in a run of
            k + 1 equal bytes and T goes on with it.  A compare that is not stopped at in_len lengthens the last match into T.
  front     F is the BAIT bytes directly in front of in - dict_len and ends with (P + T)[:300], so that the stream's beginning
            repeats at distance 300 + len(H) from `in`.  A finder that enters or probes positions in front of the history then
            emits a distance no reader accepts (or, behind a shared dictionary object, one that reads other bytes).
  body      seeded word text with a few runs: compressible, so that the finders are busy.
  tiny      n < 2 k + 8 cannot hold the repeat: T continues P's last byte at distance 1, the bait property is not asked.

Lengths: every n in 0..40, and n = e - 17 .. e + 17 around each edge e at which an engine's end-of-input path changes -- 256
(level-1 class batch), 1024 (rows batch), 4096 (Z_RLE batch), 61440 (block), 131072 (segment) -- thinned at the two large
edges; one stream of 300 KiB + 5 for the one-stream call (three segments).  Every list meets every start phase in % 16 and
every end phase (in + in_len) % 16 in the tiny group and in the union of the edge groups (coverage() is the table;
test_surround_cases_cpu.py asserts it).

Layouts: the same placements three times in one image -- "zeros" (F and T zero: the layout every older test uses), "bait",
"noise" (F and T seeded random bytes XOR 0xFF).  At least MARGIN = 4096 bytes of the image lie in front of every F and behind
every T: whatever a wrong kernel reads, it reads inside the allocation, and shows in the output, never as a fault."""
import collections
import functools
import zlib

import numpy as np

MARGIN, BAIT, FRONT_COPY = 4096, 600, 300
K_MIN = 8
MAX_DIST = 32768 - 262
DISTANCES = (1, 2, 3, 8, 64, 300, 4096)
D_LARGE = MAX_DIST
SMALL_EDGES, LARGE_EDGES = (256, 1024, 4096), (61440, 131072)
EDGES = SMALL_EDGES + LARGE_EDGES
DICT_LENS = (0, 1, 5, 300, 32768)
ONE_STREAM = (300 << 10) + 5
ONE_PHASES = (0, 1, 7, 15)
STORED_EDGES = (65535, 131070)
WINDOW_CAP = {9: 250, 12: 3834, 15: MAX_DIST}
LAYOUTS = ("zeros", "bait", "noise")
LISTS = ("main", "dict", "win9", "win12", "stored", "one")
# (group, n, D, dict_len, seed) -> k, where zlib's level 1 declines the case with the k it would get: a chance match of the
# word text ends exactly at len(P), so no token reaches across it (test_surround_cases_cpu.py::test_zlib_takes_the_bait)
K_ADJUSTED = {("e61440", 61456, 8, 0, 0): 9, ("s65535", 65533, 8, 0, 3): 9, ("s131070", 131069, 300, 0, 3): 9}


class Case:
    """H, P, F, T as above; D, k: the repeat P ends in (tiny: D = 1 and no promise); group: 'tiny', 'e256' ...; unique: the
    repeated bytes occur nowhere else in H + P (the cases whose D lies just above a window cap: they must come out as literals)"""

    def __init__(self, group, n, D, k, H, P, F, T, tiny, unique, seed):
        self.group, self.n, self.D, self.k, self.tiny, self.unique = group, n, D, k, tiny, unique
        self.H, self.P, self.F, self.T = bytes(H), bytes(P), bytes(F), bytes(T)
        self.name = "%s/n%d-D%d-k%d-dict%d-s%d%s" % (group, n, D, k, len(H), seed, "-unique" if unique else "")

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _vocabulary():
    rng = np.random.default_rng(0x5352)
    return [bytes(rng.integers(97, 123, size=int(m), dtype=np.uint8)) for m in rng.integers(2, 10, size=256)]


def body(n, rng):
    """n bytes of word text over a fixed vocabulary of 256 words, with a few runs of one letter"""
    words = _vocabulary()
    if n == 0:
        return bytearray()
    pick = rng.integers(0, 256, size=n // 3 + 2)
    text = bytearray(b" ".join(words[int(i)] for i in pick)[:n])
    assert len(text) == n
    for _ in range(min(3 + n // 20000, n // 100)):
        at, m = int(rng.integers(0, n)), int(rng.integers(5, 41))
        text[at:at + m] = bytes([int(rng.integers(97, 123))]) * len(text[at:at + m])
    return text


@functools.lru_cache(maxsize=None)
def make_case(group, n, D, k, dict_len, seed, unique=False):
    """one case; D None: a tiny one.  The repeat's source lies inside P (k + D <= n), as the property is stated."""
    k = K_ADJUSTED.get((group, n, D, dict_len, seed), k)
    rng = np.random.default_rng([0x5352, n, dict_len, seed])
    S = body(dict_len + n, rng)
    tiny = D is None
    if tiny:
        D, k = 1, 0
    else:
        assert k >= K_MIN and n >= 2 * k + 8 and k + D <= n, (n, D, k)
        if unique:                                         # the source of the repeat: bytes no word text holds
            lo = dict_len + n - k - D
            S[lo:lo + min(k, D)] = bytes(rng.permutation(np.arange(128, 256, dtype=np.uint8))[:min(k, D)])
        for i in range(dict_len + n - k, dict_len + n):
            S[i] = S[i - D]
    H, P = S[:dict_len], S[dict_len:]
    W = bytearray(P)
    for _ in range(BAIT):
        W.append(W[-D] if len(W) >= D else (H[-1] if H else 0x61))
    T = W[n:]
    F = body(BAIT - FRONT_COPY, np.random.default_rng([0x4652, zlib.crc32(bytes(S))])) + W[:FRONT_COPY]
    assert len(F) == BAIT and len(T) == BAIT
    return Case(group, n, D, k, H, P, F, T, tiny, unique, seed)


def bait_property(c):
    """the tail and front promises, from the definitions, on the case's bytes alone"""
    W = c.P + c.T
    n = len(c.P)
    tail = (c.k >= K_MIN and n >= c.k + c.D and c.P[n - c.k:] == c.P[n - c.k - c.D:n - c.D]
            and len(c.T) >= BAIT and all(c.T[j] == W[n + j - c.D] for j in range(len(c.T))))
    if c.D == 1:
        tail = tail and len(set(c.P[-4:])) == 1 and c.T[0] == c.P[-1]
    front = len(c.F) == BAIT and c.F[BAIT - FRONT_COPY:] == W[:FRONT_COPY] and c.F[BAIT - FRONT_COPY:][:min(n, FRONT_COPY)] == c.P[:FRONT_COPY]
    return bool(tail and front)


Placement = collections.namedtuple("Placement", "case phase")


def _feasible(n, dists, k=K_MIN):
    return [d for d in dists if d + k <= n]


def _list(dists, large_dists, dict_lens, above=()):
    """placements of one engine's list.  dists: the distances of the small groups, large_dists: of the two large edges;
    dict_lens: cycled over (32768 is added at three phases when it is among them); above: (group, n, D, k, dict_len) of unique cases"""
    big_dict = 32768 in dict_lens
    dls = [d for d in dict_lens if d != 32768]
    out, idx = [], 0

    def add(group, n, dl, seed, phase, twin):
        nonlocal idx
        feas = _feasible(n, large_dists if group in ("e61440", "e131072") else dists) if n >= 2 * K_MIN + 8 else []
        D = feas[idx % len(feas)] if feas else None
        k = K_MIN + (idx % 5) * 7 if D is not None and n >= 2 * (K_MIN + 28) + 8 and D + K_MIN + 28 <= n else K_MIN
        c = make_case(group, n, D, k if D is not None else 0, dl, seed)
        out.append(Placement(c, phase % 16))
        if twin:
            out.append(Placement(c, (phase + 9) % 16))
        idx += 1

    for n in range(41):                                                        # the tiny group: four cases per length
        for rep in range(4):
            add("tiny", n, dls[(n + rep) % len(dls)], rep, 5 * idx + rep, idx % 3 == 0)
    for e in SMALL_EDGES:                                                      # e - 17 .. e + 17, one case per length
        for n in range(e - 17, e + 18):
            add("e%d" % e, n, dls[idx % len(dls)], 0, 3 * idx + 1, idx % 3 == 0)
    for e in LARGE_EDGES:                                                      # thinned: eight lengths, five phases + two twins
        for n, phase in zip((e - 17, e - 16, e - 1, e, e + 1, e + 15, e + 16, e + 17), (15, 1, 0, 7, 15, 4, 9, 2)):
            add("e%d" % e, n, dls[idx % len(dls)], 0, phase, phase in (1, 4))
    if big_dict:                                                               # the whole window as history: three phases only
        for group, n, phase in (("tiny", 33, 0), ("e1024", 1024 + 3, 5), ("e61440", 61440 - 5, 15)):
            add(group, n, 32768, 1, phase, False)
    for group, n, D, k, dl in above:
        out.append(Placement(make_case(group, n, D, k, dl, 2, unique=True), (n + D) % 16))
    return out


@functools.lru_cache(maxsize=None)
def placements(name):
    """the list of an engine:
      main    zng_rocm_deflate_quick_dev, the rows engine at every level, Z_RLE, Z_HUFFMAN_ONLY, Z_FIXED, the wrappers
      dict    the calls behind a shared dictionary object: no job has history of its own, F stands directly in front of `in`
      win9, win12   the window form: distances inside the cap, and unique cases whose D lies just above it
      stored  main and lengths around the stored block's 65535 and twice that
      one     the one-stream call: 300 KiB + 5 at four phases, without history and with 300 bytes of it"""
    small = tuple(d for d in DISTANCES)
    if name == "main":
        return _list(small, small + (D_LARGE,), DICT_LENS)
    if name == "dict":
        return _list(small, small + (D_LARGE,), (0,))
    if name in ("win9", "win12"):
        cap = WINDOW_CAP[int(name[3:])]
        inside = tuple(d for d in DISTANCES if d <= cap)
        above = {9: (("e1024", 1024 - 9, cap + 1, 40, 0), ("e4096", 4096 - 6, cap + 2, 33, 5)),
                 12: (("e4096", 4096 + 9, cap + 1, 40, 0), ("e4096", 4096 + 14, cap + 2, 33, 5))}[int(name[3:])]
        return _list(inside, inside, DICT_LENS, above=above)
    if name == "stored":
        extra, idx = [], 0
        for e in STORED_EDGES:
            for n in range(e - 2, e + 3):
                extra.append(Placement(make_case("s%d" % e, n, (8, 300, 4096, D_LARGE, 1)[idx % 5], K_MIN, (0, 5)[idx % 2], 3), (7 * idx + 15) % 16))
                idx += 1
        return placements("main") + extra
    if name == "one":
        return [Placement(make_case("one", ONE_STREAM, D_LARGE, 36, dl, 4), ph) for dl in (0, 300) for ph in ONE_PHASES]
    raise KeyError(name)


def coverage(pl):
    """{'tiny' | 'edges': (set of start phases, set of end phases)} and {large edge: set of start phases} of a placement list"""
    table = {"tiny": (set(), set()), "edges": (set(), set())}
    large = {e: set() for e in LARGE_EDGES}
    for c, phase in pl:
        if c.group == "tiny" or c.group.startswith("e"):
            s, e = table["tiny" if c.group == "tiny" else "edges"]
            s.add(phase)
            e.add((phase + c.n) % 16)
        for edge in LARGE_EDGES:
            if c.group == "e%d" % edge:
                large[edge].add(phase)
    return table, large


class Job:
    """one placement in one layout: stream = image[in_off : in_off + n], its history in front of it; key: index of the
    case among the list's distinct cases (jobs with one key must give the same bytes)"""

    def __init__(self, case, phase, layout, in_off, key):
        self.case, self.phase, self.layout, self.in_off, self.key = case, phase, layout, in_off, key


class Image:
    """host: the uint8 image; jobs: every placement in every layout asked for, layout-major"""

    def __init__(self, host, jobs):
        self.host, self.jobs = host, jobs


def build_image(pl, layouts=LAYOUTS, history=True):
    """history False: H is not laid down and F stands directly in front of `in` (the shared-dictionary calls; the list's
    cases have no H then)"""
    keys, spans, pos = {}, [], 0
    for layout in layouts:
        for c, phase in pl:
            hl = len(c.H) if history else 0
            assert history or not c.H
            at = pos + MARGIN + BAIT + hl
            at += (phase - at) % 16
            spans.append((c, phase, layout, at, keys.setdefault(c.name, len(keys))))
            pos = at + c.n + BAIT
    total = pos + MARGIN
    noise = np.random.default_rng(0x4E4F).integers(0, 256, size=total, dtype=np.uint8) ^ 0xFF
    host = np.zeros(total, dtype=np.uint8)
    jobs = []
    for c, phase, layout, at, key in spans:
        hl = len(c.H) if history else 0
        lo, hi = at - hl - BAIT, at + c.n + BAIT
        if layout == "noise":                                  # the margins as well: nothing friendly anywhere near
            host[lo - MARGIN // 2:hi + MARGIN // 2] = noise[lo - MARGIN // 2:hi + MARGIN // 2]
        elif layout == "bait":
            host[lo:lo + BAIT] = np.frombuffer(c.F, dtype=np.uint8)
            host[hi - BAIT:hi] = np.frombuffer(c.T, dtype=np.uint8)
        host[at - hl:at + c.n] = np.frombuffer((c.H if history else b"") + c.P, dtype=np.uint8)
        assert at % 16 == phase
        jobs.append(Job(c, phase, layout, at, key))
    return Image(host, jobs)
