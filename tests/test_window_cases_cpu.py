"""No GPU: the generators of tests/window_cases.py keep their promises, and CPython's zlib at wbits = -w shows the recall and
the cap that tests/test_gpu_deflate_window.py asks of the device at the same window -- so every cell there is one a reference
compressor with that window covers, at distance exactly D, and every too-far cell one it leaves as literals."""
import zlib

import pytest

import deflate_parse as dp
import matcher_cases as mc
import window_cases as wc


def test_cap_table():
    assert [wc.cap(w) for w in wc.WINDOWS] == [250, 762, 1786, 3834, 7930, 16122]
    assert wc.cap(15) == mc.MAX_DIST


@pytest.mark.parametrize("w", wc.WINDOWS)
def test_cells_keep_their_promises(w):
    cells = wc.cells(w)
    seen = set()
    for c in cells:
        both = c.history + c.data
        at = len(c.history) + c.at
        assert both[at:at + c.m] == both[at - c.D:at - c.D + c.m], c.name          # the copy lies D back
        assert c.too_far == (c.D > wc.cap(w)) and c.near == (c.D < c.m)
        if not c.near:                                                             # ... and nowhere else: R's strings are distinct
            r = both[at:at + c.m]
            assert both.count(r[:4]) == 2, c.name
        assert 0 not in both[at:at + c.m]
        seen.add((c.sweep, c.m, c.D))
    for m in wc.LENGTHS:
        for D in (1, 7, wc.cap(w) - 1, wc.cap(w)):
            assert ("pos", m, D) in seen
        for D in (wc.cap(w) + 1, 1 << w, 32506):
            assert ("far", m, D) in seen
    # the priming cell: the source begins exactly cap in front of the second segment's first byte
    assert any(c.sweep == "pos" and c.at == mc.SEGMENT and c.D == wc.cap(w) for c in cells)
    # behind the long history most of it lies beyond the window, and the stream begins with R
    assert any(c.sweep == "dict" and len(c.history) == 32768 and c.at == 0 and not c.too_far for c in cells)
    host, offs, lens, dls = mc.pack([(c.history, c.data) for c in cells])
    assert host.size < 32 << 20 and all(o % 16 == 0 for o in offs)


def _cpython(c, level):
    if c.history:
        z = zlib.compressobj(level, zlib.DEFLATED, -c.w, 8, zlib.Z_DEFAULT_STRATEGY, c.history)
    else:
        z = zlib.compressobj(level, zlib.DEFLATED, -c.w)
    return z.compress(c.data) + z.flush()


@pytest.mark.parametrize("level", (1, 6, 9))
@pytest.mark.parametrize("w", wc.WINDOWS)
def test_cpython_shows_recall_and_cap(w, level):
    """every cell of the GPU test: CPython at this window covers the range by the rule the device is held to (at most 3
    literal bytes, every match at distance D, or a multiple of D in the near form), never exceeds the cap, and leaves the
    too-far ranges as literals; its own small-window reader takes the stream.  The pairs it misses are exactly
    window_cases.cpython_misses: none is dropped that it covers."""
    bad = []
    for c in wc.cells(w):
        comp = _cpython(c, level)
        p = dp.parse(comp, history=c.history)
        assert p.data == c.data
        assert wc.reader(-w, comp, zdict=c.history or None) == (c.data, True, b""), c.name
        wrong = wc.limits(c, p)
        if wrong:
            bad.append((c.name, wrong))
        elif not c.too_far:
            # CPython has one segment: a range is judged whole, not cut at 131072
            got, ok = wc.recall(c, p, split=False)
            if ok == wc.cpython_misses(c, level):
                bad.append((c.name, got, "covered, but listed as a miss" if ok else "missed"))
    assert not bad, bad


@pytest.mark.parametrize("level", (1, 6, 9))
@pytest.mark.parametrize("w", wc.WINDOWS)
def test_cpython_at_the_cap_exactly(w, level):
    """m = 64 at 40000: D = cap is covered with no literal byte at distance exactly cap; D = cap + 1 and D = 1 << w are
    literals throughout"""
    for D in (wc.cap(w), wc.cap(w) + 1, 1 << w):
        c = wc.planted(w, 64, D, 40000)
        cov = mc.coverage(dp.parse(_cpython(c, level)), c.at, c.at + c.m)
        if D == wc.cap(w):
            assert (cov.lits, cov.dists) == (0, {D}), (c.name, cov)
        else:
            assert (cov.lits, cov.dists) == (64, set()), (c.name, cov)
        assert cov.max_dist <= wc.cap(w)


def test_whole_buffer_decode_proves_nothing():
    """why the reader is fed in pieces: a distance-600 stream is refused by a 512-byte window only when copies go through it"""
    c = mc.planted("demo", 64, 600, 4000, 300)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = z.compress(c.data) + z.flush()
    assert 600 in mc.coverage(dp.parse(comp), c.at, c.at + c.m).dists
    with pytest.raises(zlib.error, match="invalid distance too far back"):
        wc.reader(-9, comp, chunk=64)
    assert wc.reader(-10, comp, chunk=64)[0] == c.data
    assert wc.reader(-15, comp, chunk=64)[0] == c.data
