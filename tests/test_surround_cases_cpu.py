"""CPU: the builder of tests/surround_cases.py is held to its promises, and CPython's zlib to taking the bait.

  * the bait property holds for every non-tiny case of every list, asserted on the bytes with the definitions of the builder's
    docstring; every case's F and T are functions of H and P alone (the builder is seeded by them);
  * the phase table of every engine's list is complete: every start phase and every end phase in the tiny group and in the union
    of the edge groups, at least four start phases with an odd one and 15 at each of the two large edges, the whole window as
    history at three phases, every required distance, D = 1 among them;
  * the three layouts hold the same streams at the same places, differ only in F and T (and, for "noise", the margins), and keep
    4 KiB of the image around every case;
  * zlib at levels 1 and 6 (raw, zdict = H) compresses every P and P + T[:258]: in the second stream the token that covers the
    last byte of P is a match that reaches across len(P), and at least 200 of the 258 bait bytes lie in matches whose distance
    is a multiple of the bait's period -- the continuation of the repeat, not a chance match of the word text.  (The stream's
    very last token cannot be the one that reaches across len(P): the repeat is k + 258 bytes long by then and a match holds
    258.)  zlib's own finder stops one short of MAX_DIST (cur_match > limit, deflate's longest_match), so it cannot take a
    repeat of distance 32506 itself: those cases are held to the first half alone.  So the bait is something a real matcher
    takes -- shown on the reference, not on the device.  tests/deflate_parse.py reads the tokens.  Three cases that level 1
    declined got another k (surround_cases.K_ADJUSTED)."""
import zlib

import numpy as np
import pytest

import deflate_parse as dp
import surround_cases as sc


def _distinct(name):
    seen = {}
    for c, _ in sc.placements(name):
        seen.setdefault(c.name, c)
    return list(seen.values())


@pytest.mark.parametrize("name", sc.LISTS)
def test_bait_property_holds_for_every_non_tiny_case(name):
    cases = _distinct(name)
    for c in cases:
        assert c.tiny == (c.n < 2 * sc.K_MIN + 8), c
        if not c.tiny:
            assert sc.bait_property(c), c
        else:
            assert len(c.T) == sc.BAIT and len(set(c.T)) == 1 and (not c.P or c.T[0] == c.P[-1]), c
        again = sc.make_case.__wrapped__(c.group, c.n, None if c.tiny else c.D, c.k, len(c.H), int(c.name.split("-s")[1].split("-")[0]), c.unique)
        assert (again.H, again.P, again.F, again.T) == (c.H, c.P, c.F, c.T), c
    assert sum(not c.tiny for c in cases) >= (2 if name == "one" else 150)


@pytest.mark.parametrize("name", [n for n in sc.LISTS if n != "one"])
def test_phase_table_is_complete(name):
    pl = sc.placements(name)
    table, large = sc.coverage(pl)
    every = set(range(16))
    for group in ("tiny", "edges"):
        assert table[group][0] == every, (group, "start phases")
        assert table[group][1] == every, (group, "end phases")
    for edge, phases in large.items():
        assert len(phases) >= 4 and 15 in phases and any(p % 2 for p in phases), edge
    assert {c.n for c, _ in pl if c.group == "tiny"} == set(range(41))
    for e in sc.SMALL_EDGES:
        assert {c.n for c, _ in pl if c.group == "e%d" % e} >= set(range(e - 17, e + 18))
    for e in sc.LARGE_EDGES:
        assert {c.n - e for c, _ in pl if c.group == "e%d" % e} >= {-17, -16, -1, 0, 1, 15, 16, 17}
    dists = {c.D for c, _ in pl if not c.tiny}
    if name in ("main", "dict", "stored"):
        assert dists >= set(sc.DISTANCES) | {sc.D_LARGE}
        assert all(c.D != sc.D_LARGE or c.n > 60000 for c, _ in pl)
    else:
        cap = sc.WINDOW_CAP[int(name[3:])]
        assert dists >= {d for d in sc.DISTANCES if d <= cap} | {cap + 1}
        assert all(c.unique == (c.D > cap) for c, _ in pl)
    assert 1 in dists
    dls = {len(c.H) for c, _ in pl}
    assert dls == ({0} if name == "dict" else set(sc.DICT_LENS))
    if name != "dict":
        assert len({ph for c, ph in pl if len(c.H) == 32768}) == 3 == sum(len(c.H) == 32768 for c, _ in pl)
    twins = {}
    for c, ph in pl:
        twins.setdefault(c.name, set()).add(ph)
    assert sum(len(v) == 2 for v in twins.values()) >= 60                      # the same (H, P) at two phases


def test_lists_of_the_one_stream_call_and_of_level_0():
    one = sc.placements("one")
    assert {(len(c.H), ph) for c, ph in one} == {(dl, ph) for dl in (0, 300) for ph in sc.ONE_PHASES}
    assert all(c.n == sc.ONE_STREAM and c.n > 2 * 131072 for c, _ in one)
    stored = {c.n for c, _ in sc.placements("stored")}
    for e in sc.STORED_EDGES:
        assert stored >= set(range(e - 2, e + 3))


def test_layouts_differ_in_the_surroundings_alone():
    pl = sc.placements("main")
    im = sc.build_image(pl)
    per = len(pl)
    assert len(im.jobs) == 3 * per and [j.layout for j in im.jobs[::per]] == list(sc.LAYOUTS)
    host = im.host
    end = 0
    for j in im.jobs:
        c, at = j.case, j.in_off
        lo, hi = at - len(c.H) - sc.BAIT, at + c.n + sc.BAIT
        assert at % 16 == j.phase and lo - end >= sc.MARGIN and hi + sc.MARGIN <= host.size, c
        end = hi
        assert host[at - len(c.H):at + c.n].tobytes() == c.H + c.P, c
        front, tail = host[lo:lo + sc.BAIT].tobytes(), host[hi - sc.BAIT:hi].tobytes()
        if j.layout == "zeros":
            assert front == bytes(sc.BAIT) == tail and not host[lo - sc.MARGIN:lo].any() and not host[hi:hi + sc.MARGIN].any()
        elif j.layout == "bait":
            assert (front, tail) == (c.F, c.T)
        else:
            assert front != c.F and tail != c.T and len(set(front)) > 100 and len(set(tail)) > 100
    keys = {}
    for j in im.jobs:
        keys.setdefault(j.key, set()).add(j.case.name)
    assert all(len(v) == 1 for v in keys.values()) and len(keys) == len({c.name for c, _ in pl})
    shared = sc.build_image(sc.placements("dict"), layouts=("bait",), history=False)
    for j in shared.jobs[:40]:
        assert shared.host[j.in_off - sc.BAIT:j.in_off].tobytes() == j.case.F


def _tokens(stream, history):
    """[(start, end, is_match, distance)] of every token"""
    out = []
    for b in dp.parse(stream, history=history).blocks:
        pos = b.out_start
        if b.btype == dp.STORED:
            out += [(p, p + 1, False, 0) for p in range(b.out_start, b.out_end)]
            continue
        at = {m[0]: m for m in b.matches}
        for i, s in enumerate(b.lit_syms):
            if s < 256:
                out.append((pos, pos + 1, False, 0))
                pos += 1
            elif s > 256:
                out.append((pos, pos + at[i][1], True, at[i][2]))
                pos += at[i][1]
    return out


def _deflate(level, data, history):
    co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, history) if history else \
        zlib.compressobj(level, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY)
    return co.compress(data) + co.flush()


@pytest.mark.parametrize("level", (1, 6))
def test_zlib_takes_the_bait(level):
    seen = set()
    for name in sc.LISTS:
        for c in _distinct(name):
            if c.name in seen:
                continue
            seen.add(c.name)
            hist = c.H[-32768:]
            alone = _deflate(level, c.P, hist)
            d = zlib.decompressobj(-15, zdict=hist) if hist else zlib.decompressobj(-15)
            assert d.decompress(alone) == c.P and d.eof, c
            if c.tiny:
                continue
            toks = _tokens(_deflate(level, c.P + c.T[:258], hist), hist)
            assert toks[-1][1] == c.n + 258, c
            across = [t for t in toks if t[0] < c.n < t[1]]
            assert len(across) == 1 and across[0][2], (c, across)
            if c.D == sc.D_LARGE:
                continue
            period = next((p for p in range(1, sc.BAIT // 2) if c.T[p:] == c.T[:-p]), c.D)
            taken = sum(min(t[1], c.n + 258) - max(t[0], c.n) for t in toks if t[2] and t[3] % period == 0 and t[1] > c.n)
            assert taken >= 200, (c, period, taken)
