"""CPU: the planted-repeat generators of tests/matcher_cases.py keep their promises, and the reference side -- CPython's
zlib, taken apart by tests/deflate_parse.py -- meets the recall that tests/test_gpu_matcher_recall.py asks of the device:
level 6 for the cells of the rows class, level 1 for those of the level-1 class.  This is the precondition of the GPU file:
a cell in which a serial chain matcher could not cover the range would say nothing about the device's finders."""
import zlib

import pytest

import deflate_parse as dp
import matcher_cases as mc

CELLS = mc.cells()
SWEEPS = ("dist", "pos", "len", "tail", "dict")


def _zlib_raw(data, level, history=b""):
    if history:
        c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY, history)
    else:
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
    return c.compress(data) + c.flush()


def _occurrences(hay, needle, end):
    """every start below `end` at which `needle` occurs in `hay`"""
    out, i = [], hay.find(needle)
    while 0 <= i < end:
        out.append(i)
        i = hay.find(needle, i + 1)
    return out


def test_the_cells_are_the_sweeps_of_the_issue():
    by = {s: [c for c in CELLS if c.sweep == s] for s in SWEEPS}
    assert sum(len(v) for v in by.values()) == len(CELLS) and 230 <= len(CELLS) <= 300
    assert {(c.m, c.D) for c in by["dist"]} == {(m, D) for m in (16, 64, 300) for D in mc.DISTANCES + mc.TOO_FAR}
    assert {c.D for c in CELLS if c.too_far} == set(mc.TOO_FAR)
    assert {(c.m, c.D) for c in by["len"]} == {(m, D) for m in mc.LENGTHS for D in (3, 4096)}
    assert {(c.m, c.D, c.tail) for c in by["tail"]} == {(m, D, t) for m in (16, 300) for D in (7, 4096) for t in mc.TAILS}
    assert {(len(c.history), c.at) for c in by["dict"]} == {(d, o) for d in mc.DICT_LENS for o in mc.DICT_OFFS}
    assert mc.BORDERS == (4160, 5120, 61440, 131072)
    for b in mc.BORDERS:                                     # every border from every side, a 258-byte range across it
        at = {c.at - b for c in by["pos"] if abs(c.at - b) <= 130}
        assert at == {-130, -1, 0, 1}, b
        assert any(c.at < b < c.at + c.m and c.m >= 258 for c in by["pos"])
    assert any(mc.segment_border(c) and c.D == mc.MAX_DIST for c in by["pos"])      # reached through the priming only
    assert all(len(c.data) <= 165 << 10 for c in CELLS)
    assert sum(len(c.data) + len(c.history) for c in CELLS) < 32 << 20              # one call: 128 KiB segments


@pytest.mark.parametrize("sweep", SWEEPS)
def test_generator_promises(sweep):
    """positions and lengths as stated; the four-byte strings of R distinct; exactly one earlier copy of the range, at
    distance D (far form) -- or copies at multiples of D only (near form); nothing but zeros around it"""
    for c in (c for c in CELLS if c.sweep == sweep):
        both = c.history + c.data
        h, at, m, D = len(c.history), len(c.history) + c.at, c.m, c.D
        assert len(c.data) == c.at + m + c.tail and at >= D, c.name
        rng = both[at:at + m]
        assert 0 not in rng and both[at - D:at - D + m] == rng, c.name
        assert not any(both[at + m:]), c.name
        if not c.near:
            assert len(set(mc._grams(rng))) == m - 3, c.name
            assert not any(both[:at - D]) and not any(both[at - D + m:at]), c.name
            for i in range(0, m - 3):
                assert _occurrences(both, rng[i:i + 4], at + i + 1) == [at - D + i, at + i], (c.name, i)
        else:
            assert not any(both[:at - D]) and 0 not in both[at - D:at], c.name
            assert len(set(mc._grams(both[at - D:at + 3]))) == D, c.name
            for i in range(0, min(m - 3, 2 * D)):
                occ = _occurrences(both, rng[i:i + 4], at + i + 1)
                assert occ[-1] == at + i and all((at + i - o) % D == 0 for o in occ), (c.name, i)
                assert occ[0] == at - D + i % D, (c.name, i)
        if c.history:
            assert len(c.history) in mc.DICT_LENS and at - D + m <= h, c.name          # the source lies in the dictionary
            assert at - D == 0 or D == mc.MAX_DIST, c.name                            # at its first bytes where D allows


@pytest.mark.parametrize("level,sweep", [(lv, s) for lv in (6, 1) for s in SWEEPS])
def test_zlib_meets_the_recall(level, sweep):
    worst = (0, "")
    for c in (c for c in CELLS if c.sweep == sweep):
        p = dp.parse(_zlib_raw(c.data, level, c.history), history=c.history)
        assert p.data == c.data
        cov = mc.coverage(p, c.at, c.at + c.m, len(c.history))
        assert cov.max_dist <= mc.MAX_DIST and cov.min_reach >= 0, c.name
        if c.too_far:
            assert cov.lits == c.m and not cov.dists, (c.name, cov)
            continue
        worst = max(worst, (cov.lits, c.name))
        assert cov.lits <= 3, (c.name, cov)
        assert cov.dists and all(d % c.D == 0 if c.near else d == c.D for d in cov.dists), (c.name, cov)
    print("zlib level %d, %s sweep: worst cell %s with %d literal bytes" % (level, sweep, worst[1], worst[0]))


def test_coverage_walks_positions():
    """the walker on a stream written by hand: literals, a match across the range's edge, a stored block"""
    import deflate_craft as craft
    bits = craft.Bits()
    craft.fixed_block(bits, [("L", 1), ("L", 2), ("L", 3), ("L", 4), ("L", 5), ("M", 4, 5), ("L", 9), ("M", 3, 2)], False)
    craft.stored_block(bits, bytes([7, 7, 7]), False)
    craft.fixed_block(bits, [("M", 5, 16), ("L", 8)], True)
    bits.align()
    p = dp.parse(bytes(bits.out))
    assert p.data == bytes([1, 2, 3, 4, 5, 1, 2, 3, 4, 9, 4, 9, 4, 7, 7, 7, 1, 2, 3, 4, 5, 8])
    assert mc.coverage(p, 5, 9) == mc.Cover(0, {5}, 16, 0, 1)
    assert mc.coverage(p, 4, 10) == mc.Cover(2, {5}, 16, 0, 3)
    assert mc.coverage(p, 10, 13) == mc.Cover(0, {2}, 16, 0, 1)
    assert mc.coverage(p, 12, 17) == mc.Cover(3, {2, 16}, 16, 0, 5)        # the stored block's bytes count as literals
    assert mc.coverage(p, 21, 22) == mc.Cover(1, set(), 16, 0, 1)
    assert mc.coverage(p, 0, 22, hist_len=4).min_reach == 4                # history in front: positions count from its first byte


def test_budget_streams():
    """k + 1 strings with the query's first four bytes inside MAX_DIST in front of it, each more than a batch before the
    next; `rot` more beyond MAX_DIST; only the true source goes on; zlib level 6 covers the query from its first byte"""
    streams = mc.budget_streams()
    assert sorted({s.k for s in streams}) == [0, 1, 2, 5, 7] and {s.rot for s in streams} == set(range(8))
    for s in streams:
        q, xt = s.query, s.x + s.t
        assert s.data[q:q + 204] == xt and s.data[q - s.dist:q - s.dist + 204] == xt
        occ = _occurrences(s.data, s.x, q)
        near = [o for o in occ if q - o <= mc.MAX_DIST]
        assert len(occ) == s.rot + s.k + 1 and len(near) == s.k + 1 and near[0] == q - s.dist, s.name
        assert all(q - 3 - o > mc.MAX_DIST for o in occ[:s.rot]), s.name
        assert all(b - a >= mc.GAP for a, b in zip(occ + [q], (occ + [q])[1:])), s.name
        assert all(s.data[o + 4] != s.t[0] for o in occ if o != q - s.dist), s.name
        assert _occurrences(s.data, xt[1:5], q + 2) == [q - s.dist + 1, q + 1], s.name     # one byte later: unique
        p = dp.parse(_zlib_raw(s.data, 6))
        cov = mc.coverage(p, q, q + 200)
        assert cov.lits == 0 and cov.dists == {s.dist}, (s.name, cov)
