"""The crafted runs of tests/rle_cases.py are what they claim, without a GPU: for every case and every segment the closed form
rle_rows_kernel evaluates (strategy_util.rle_closed_form) equals the greedy parse (rle_parse); every case reaches the edge it
was built for -- derived here from the model's token starts and the input's breaks, never from the product --; and CPython's
own Z_RLE writes the expected tokens for every case that is one segment, with its history as zdict."""
import collections
import zlib

import numpy as np
import pytest

import rle_cases as rc
import strategy_util as su
from rle_cases import BATCH, BLOCK, CHAIN, LANE, SEGMENT, ALIGN


def _arrays(case):
    """(tok, mat) over every position of history + data, from the greedy parse"""
    n = len(case.history) + len(case.data)
    tok, mat = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for p, t in rc.token_starts(case):
        tok[p] = True
        mat[p] = t[0] == 'm'
    return tok, mat


def _run_end(brk, p):
    """the first break behind p, or the end"""
    later = np.flatnonzero(brk[p + 1:])
    return p + 1 + int(later[0]) if later.size else brk.size


def test_counts_and_sizes():
    count = collections.Counter(c.family for c in rc.cases())
    print("rle cases per family: " + ", ".join("%s %d" % (f, count[f]) for f in rc.FAMILIES) + "; %d in all, %d bytes"
          % (len(rc.cases()), sum(len(c.history) + len(c.data) for c in rc.cases())))
    assert all(count[f] for f in rc.FAMILIES)
    assert sum(len(c.data) < SEGMENT + 8192 for c in rc.cases()) > len(rc.cases()) * 0.9
    for c in rc.cases():
        alphabet = set(c.data) | set(c.history)
        if c.family != "plain":
            assert alphabet <= set(rc.NOISE) | set(rc.RUN) | set(rc.FILL), c.name


def test_noise_is_breaks_throughout():
    for n in (0, 1, 2, 1000, 70000):
        d = np.frombuffer(rc.noise(n, 5), dtype=np.uint8)
        assert d.size == n and np.all(d[1:] != d[:-1]) and set(d.tolist()) <= set(rc.NOISE)
    f = rc.filler(50000, 3)
    assert len(f) == 50000 and set(f) <= set(rc.NOISE) | set(rc.FILL)


def test_closed_form_equals_the_greedy_parse():
    for c in rc.cases():
        both = c.history + c.data
        tok, mat = _arrays(c)
        for a, b in rc.segments(c):
            ctok, cmat = su.rle_closed_form(both, a, b)
            assert np.array_equal(ctok, tok[a:b]) and np.array_equal(cmat, mat[a:b]), (c.name, a, b)


def test_expected_tokens_spell_the_data():
    for c in rc.cases():
        n = sum(t[1] if t[0] == 'm' else 1 for t in rc.expected_tokens(c))
        assert n == len(c.data), c.name
        ranges = rc.block_ranges(c)
        assert ranges[0][0] == c.dict_len and ranges[-1][1] == c.dict_len + len(c.data)
        assert all(lo < hi for lo, hi in ranges) or not c.data
        assert all(x[1] == y[0] for x, y in zip(ranges, ranges[1:]))


# ---- every case reaches its edge ---------------------------------------------------------------------------------------------
def _edge_carry(c, e, brk, tok, mat, toks):
    s, L = e["start"], e["length"]
    assert brk[s] and brk[s + L] and not brk[s + 1:s + L].any()
    borders = [P for P in rc.batch_borders(c) if s < P < s + L]
    assert len(borders) == e["borders"] >= 1                           # those batches' first lane has no break in front: carry_o
    whole = [P for P in borders if P + BATCH <= s + L]
    assert all(tok[P:P + BATCH].any() and mat[P:P + BATCH].sum() >= BATCH // CHAIN - 1 for P in whole)
    if L >= 2 * BATCH + CHAIN - 1:
        assert whole, "no whole batch inside the run"
    return {("phase", (P - s - 1) % CHAIN) for P in borders} | {("batches", len(borders))}


def _edge_nocarry(c, e, brk, tok, mat, toks):
    s, L = e["start"], e["length"]
    assert brk[s] and brk[s + L] and not brk[s + 1:s + L].any()
    assert s + L in (BATCH - 1, BATCH)                                 # the run's end is the batch's last or the next one's first
    return {("nocarry", s + L - BATCH)}


def _edge_tail(c, e, brk, tok, mat, toks):
    s, end, point, r, B = e["start"], e["end"], e["point"], e["r"], e["border"]
    assert brk[s] and brk[end] and not brk[s + 1:end].any()
    assert (point - (s + 1)) % CHAIN == 0 and end - point == r and abs(end - B) <= 3
    if r == 0:
        assert toks[point - CHAIN] == ('m', CHAIN, 1) and not tok[point - CHAIN + 1:end].any() and tok[end]
    elif r == 3:
        assert toks[point] == ('m', 3, 1) and not tok[point + 1:end].any()
    else:
        assert tok[point:end].all() and not mat[point:end].any()
    kinds = set()
    if r >= 1 and point == B - 1:
        kinds.add((e["which"], "chain point on the last position"))
    if r == 2 and point + 1 == B:
        kinds.add((e["which"], "second literal on the first position"))
    if r == 3 and point < B < point + 3:
        kinds.add((e["which"], "3-byte match over the border"))
    return kinds


def _edge_ahead(c, e, brk, tok, mat, toks):
    p, end, P = e["point"], e["end"], e["border"]
    assert P in rc.batch_borders(c) + [b for _, b in rc.segments(c)] and 1 <= P - p <= CHAIN and p < P <= end
    assert brk[p - 1] and not brk[p:end].any()
    stop = _run_end(brk, p)
    if e["limit"] == "segment":
        assert stop > end == P and (P - c.dict_len) % SEGMENT == 0
    else:
        assert stop == end and (end == brk.size) == (e["limit"] == "stream")
    # no break between the chain point and the border: the kernel's suffix scan finds none, the length is read ahead
    if e["match"]:
        assert toks[p] == ('m', end - p, 1)
    else:
        assert toks[p][0] == 'l' and end - p < 3
    lim = min(p + CHAIN, brk.size if e["limit"] != "segment" else P)
    if not e["match"] or p + CHAIN <= P:
        return {"no read-ahead"}
    if end + LANE <= lim and end - P < LANE:
        return {"first group"}
    if end + LANE <= lim:
        return {"later group"}
    return {"byte tail at the cap" if end == p + CHAIN else "byte tail at the " + e["limit"]}


def _edge_segment(c, e, brk, tok, mat, toks):
    s, B, r, t = e["start"], e["border"], e["r"], e["t"]
    assert (B - c.dict_len) % SEGMENT == 0 and brk[s] and not brk[s + 1:B + t].any() and (B + t == brk.size or brk[B + t])
    assert (B - (s + 1)) % CHAIN == r
    if r == 0:
        assert toks[B - CHAIN] == ('m', CHAIN, 1)
    elif r >= 3:
        assert toks[B - r] == ('m', r, 1)                              # the match ends with its segment ...
    else:
        assert tok[B - r:B].all() and not mat[B - r:B].any()
    assert tok[B]                                                      # ... and the next segment begins a token,
    assert toks[B] == (('m', min(t, CHAIN), 1) if t >= 3 else ('l', c.data[B - c.dict_len]))       # a match iff three more follow
    return {("r", min(r, 3)), ("goes on", t >= 1 and r in (0, 3) or r > 3)}


def _edge_length(c, e, brk, tok, mat, toks):
    t = e["t"]
    assert len(c.data) == SEGMENT + t and rc.segments(c)[-1] == ((SEGMENT, SEGMENT + t) if t else (0, SEGMENT))
    assert mat[SEGMENT:].sum() == (1 if t >= 3 and c.name.endswith("run") else 0)
    return {("last segment", t)}


def _edge_block(c, e, brk, tok, mat, toks):
    B, point = e["border"], e["point"]
    assert any(lo == B for lo, _ in rc.block_ranges(c))
    over = [p for p, tk in toks.items() if tk[0] == 'm' and p < B < p + tk[1]]
    if point is not None:
        assert mat[point] and not brk[point]
    assert bool(over) == (point != B)
    empty = [(lo, hi) for lo, hi in rc.block_ranges(c) if not tok[lo:hi].any()]
    assert bool(empty) == (c.name == "block/empty_last")
    return {("point", None if point is None else point - B), ("empty", bool(empty))}


def _edge_history(c, e, brk, tok, mat, toks):
    a = c.dict_len
    assert 1 <= a <= rc.HIST_MAX and e["run"] == a - 1 - int(np.flatnonzero(brk[:a])[-1]) + 1
    if e["cont"]:
        assert not brk[a]
        assert toks[a] == ('m', min(CHAIN, _run_end(brk, a) - a), 1)   # the chain's origin is a, not the run's first byte
    else:
        assert brk[a] and toks[a][0] == 'l'
    return {("phase", a % LANE), ("first < a", a % ALIGN != 0), ("segments", len(rc.segments(c)))}


def _edge_plain(c, e, brk, tok, mat, toks):
    return set()


EDGES = {"carry": _edge_carry, "nocarry": _edge_nocarry, "tail": _edge_tail, "ahead": _edge_ahead, "segment": _edge_segment,
         "length": _edge_length, "block": _edge_block, "history": _edge_history, "plain": _edge_plain}


@pytest.fixture(scope="module")
def reached():
    out = collections.defaultdict(set)
    for c in rc.cases():
        tok, mat = _arrays(c)
        try:
            out[c.edge["kind"]] |= EDGES[c.edge["kind"]](c, c.edge, rc.breaks(c), tok, mat, dict(rc.token_starts(c)))
        except AssertionError as err:
            raise AssertionError("%s does not reach its edge: %s" % (c.name, err)) from err
    return out


def test_every_case_reaches_its_edge(reached):
    for kind, what in sorted(reached.items()):
        phases = [w for w in what if w[0] == "phase"]
        print(kind, sorted(what - set(phases), key=str), "%d phases" % len(phases) if phases else "")
    # long: carry_o over 1 .. 15 batches, and the chain at many phases on a batch's first position
    assert {n for k, n in reached["carry"] if k == "batches"} >= {1, 2, 15}
    assert len({n for k, n in reached["carry"] if k == "phase"}) >= 64
    assert reached["nocarry"] == {("nocarry", -1), ("nocarry", 0)}
    # tail: the three things, on a batch, a wave and a lane border each
    for which, _ in rc.TAIL_BORDERS:
        for what in ("chain point on the last position", "second literal on the first position", "3-byte match over the border"):
            assert (which, what) in reached["tail"], (which, what)
    # ahead: the read-ahead's exits
    assert reached["ahead"] >= {"no read-ahead", "first group", "later group", "byte tail at the cap", "byte tail at the stream",
                                "byte tail at the segment"}
    assert reached["segment"] >= {("r", r) for r in range(4)} | {("goes on", True)}
    assert reached["length"] == {("last segment", t) for t in range(4)}
    assert reached["block"] >= {("point", d) for d in (None, -1, 0, 1)} | {("empty", True)}
    assert reached["history"] >= {("phase", p) for p in range(LANE)} | {("first < a", True), ("first < a", False), ("segments", 2)}


def test_second_segments_restart():
    c = rc.by_name("segment/run2seg+7")
    toks = dict(rc.token_starts(c))
    assert toks[SEGMENT] == ('m', CHAIN, 1) and toks[2 * SEGMENT] == ('m', 7, 1) and toks[0] == ('l', rc.RUN[0])
    assert toks[SEGMENT - 7] == ('m', 7, 1)
    for name in ("history/d32768-two-segments", "history/d4097-two-segments"):
        c = rc.by_name(name)
        a = c.dict_len + SEGMENT
        assert not rc.breaks(c)[a] and dict(rc.token_starts(c))[a] == ('m', CHAIN, 1)
        assert (a % ALIGN != 0) == (name == "history/d4097-two-segments")
    c = rc.by_name("block/second_segment")
    first = (c.dict_len + SEGMENT) - (c.dict_len + SEGMENT) % ALIGN
    assert first < c.dict_len + SEGMENT and c.edge["border"] == first + BLOCK


# ---- CPython's Z_RLE writes the same tokens ----------------------------------------------------------------------------------
def test_cpython_writes_the_expected_tokens():
    n = 0
    for c in rc.cases():
        if len(c.data) > SEGMENT:
            continue
        kw = {"zdict": c.history} if c.history else {}
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE, **kw)
        comp = z.compress(c.data) + z.flush()
        assert su.tokens_of(comp, window_len=len(c.history)) == rc.expected_tokens(c), c.name
        n += 1
    print("CPython agrees on %d single-segment cases" % n)
    assert n > len(rc.cases()) * 0.8
