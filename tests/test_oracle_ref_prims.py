"""Pin the oracle's deflate-side / inflate-side primitives to the reference's own compiled functions.

oracle/_ref/libzng_ref_prims.so holds slide_hash_c, the insert_string families, longest_match_c, longest_match_slow_c
and chunkmemset_safe_c of the reference, compiled with NO_UNALIGNED (OPTIMAL_CMP 8: the byte-pair probes of
match_tpl.h, the form the oracle and the kernels follow) behind oracle/ref_shim.c.  Everything here is bit-exact,
oracle against that binary; a missing binary is a failure, not a skip.

The states are in-contract (deflate_state_util.in_contract_snapshots): tables hold only positions below strstart,
before a slide with limit == 0 and limit > 0, and after a slide.
"""
import numpy as np
import pytest

import oracle_lib
from deflate_state_util import (DATA_KINDS, WINDOW_SIZES, HostState, cur_match_candidates, in_contract_snapshots,
                                limit_edge_states, match_call, match_param_sets, set_match_level, shared_slab_cases,
                                shared_slab_cases_slow, stream_data)


@pytest.fixture(scope="module")
def ref():
    return oracle_lib.load_ref_prims()


def test_reference_variant_is_byte_compare(ref):
    assert ref.ref_optimal_cmp() == 8
    assert ref.ref_chunksize() == 8


def _same_tables(a, b):
    return (a.head == b.head).all() and (a.prev == b.prev).all() and a.st.ins_h == b.st.ins_h


@pytest.mark.parametrize("kind", DATA_KINDS)
@pytest.mark.parametrize("w_size", WINDOW_SIZES)
def test_longest_match_in_contract(oracle, ref, w_size, kind):
    """longest_match at levels 1-9 and longest_match_slow at levels 7-9, every cur_match candidate and every
    (prev_length, lookahead) pair, on six snapshots of each phase; the snapshots themselves (reference's insert and
    slide) against the oracle's."""
    queries = 0
    for roll, fast_levels, slow_levels in ((False, range(1, 9), (7, 8)), (True, (9,), (9,))):
        snaps = in_contract_snapshots(ref, "ref_", kind, w_size, roll, per_phase=6)
        theirs = in_contract_snapshots(oracle, "oracle_", kind, w_size, roll, per_phase=6)
        assert [s.phase for s in snaps].count(2) >= 2 and len(snaps) == len(theirs)
        for snap, other in zip(snaps, theirs):
            assert snap.strstart == other.strstart and _same_tables(snap, other), (roll, snap.phase, snap.strstart)
            assert int(snap.head.max()) < snap.strstart                     # in contract
            curs = cur_match_candidates(snap, kind, roll)
            for name, levels in (("longest_match", fast_levels), ("longest_match_slow", slow_levels)):
                ofn, rfn = getattr(oracle, "oracle_" + name), getattr(ref, "ref_" + name)
                for level in levels:
                    set_match_level(snap, level)
                    for cur in curs:
                        for p, la in match_param_sets(level):
                            want = match_call(rfn, snap, cur, p, la)
                            got = match_call(ofn, snap, cur, p, la)
                            assert got == want, (name, level, roll, snap.phase, snap.strstart, cur, p, la)
                            queries += 1
    assert queries > 3000


@pytest.mark.parametrize("roll", [False, True])
def test_chain_ends_at_limit(oracle, ref, roll):
    """a chain whose next member lies exactly at `limit` (0 and > 0) stops there, at the probe loop's step and at the
    step after a compare: the 40-byte match at `limit` is never taken (a `>= limit` step would take it)"""
    for snap in limit_edge_states(ref, "ref_", roll):
        for name, levels in (("longest_match", (9,) if roll else range(1, 9)),
                             ("longest_match_slow", (9,) if roll else (7, 8))):
            for level in levels:
                set_match_level(snap, level)
                for p, la in ((0, 262), (2, 258), (0, 41)):
                    want = match_call(getattr(ref, "ref_" + name), snap, snap.cur, p, la)
                    assert want == (4, snap.strstart - 3)
                    assert match_call(getattr(oracle, "oracle_" + name), snap, snap.cur, p, la) == want, \
                        (name, level, snap.w_size, snap.strstart)


@pytest.mark.parametrize("level", [1, 3, 4, 6, 9])
def test_shared_slab_states_longest_match(oracle, ref, level):
    """the states test_gpu_deflate_prims.test_longest_match feeds the device (chains reach beyond strstart)"""
    hs, cases = shared_slab_cases(oracle, "oracle_", level)
    hs2, cases2 = shared_slab_cases(ref, "ref_", level)
    assert cases == cases2 and _same_tables(hs, hs2) and len(cases) > 500
    for strstart, cur, p, la in cases:
        hs.strstart = strstart
        assert match_call(oracle.oracle_longest_match, hs, cur, p, la) == \
            match_call(ref.ref_longest_match, hs, cur, p, la), (strstart, cur, p, la)


@pytest.mark.parametrize("level", [7, 8, 9])
def test_shared_slab_states_longest_match_slow(oracle, ref, level):
    """the states test_gpu_match_slow.test_longest_match_slow feeds the device"""
    hs, cases = shared_slab_cases_slow(oracle, "oracle_", level)
    hs2, cases2 = shared_slab_cases_slow(ref, "ref_", level)
    assert cases == cases2 and _same_tables(hs, hs2) and len(cases) > 1000
    for strstart, cur, p, la in cases:
        hs.strstart = strstart
        assert match_call(oracle.oracle_longest_match_slow, hs, cur, p, la) == \
            match_call(ref.ref_longest_match_slow, hs, cur, p, la), (strstart, cur, p, la)


@pytest.mark.parametrize("w_size", WINDOW_SIZES)
def test_slide_hash(oracle, ref, w_size):
    rng = np.random.default_rng(w_size)
    a = HostState(np.zeros(16, dtype=np.uint8), w_size=w_size)
    a.head[:] = rng.integers(0, 65536, size=65536, dtype=np.uint16)
    a.prev[:] = rng.integers(0, 65536, size=w_size, dtype=np.uint16)
    edges = (0, w_size - 1, w_size, w_size + 1, 65535)
    a.head[:5] = edges
    a.head[-5:] = edges
    a.prev[:5] = edges
    a.prev[-5:] = edges
    b = HostState(np.zeros(16, dtype=np.uint8), w_size=w_size)
    b.head[:], b.prev[:] = a.head, a.prev
    oracle.oracle_slide_hash(a.ref())
    ref.ref_slide_hash(b.ref())
    assert _same_tables(a, b)
    assert b.head[:5].tolist() == [0, 0, 0, 1, 65535 - w_size]


@pytest.mark.parametrize("roll", [False, True])
def test_insert_string_family(oracle, ref, roll):
    """counts 0, 1, 63, 64, 65 and 30000, positions above 32768, ins_h carried from call to call, the same position
    inserted twice; head, prev, ins_h and the returned head after every call"""
    sfx = "_roll" if roll else ""
    plans = [(0, 1), (1, 0), (1, 63), (64, 64), (128, 65), (193, 30000), (30193, 1), (32760, 65), (40000, 63),
             (50000, 12000)]
    for kind in ("texty3", "texty24", "zeros", "run3"):
        a, b = HostState(stream_data(kind, 65536)), HostState(stream_data(kind, 65536))
        a.st.ins_h = b.st.ins_h = 0x5a5a
        for start, count in plans:
            getattr(oracle, "oracle_insert_string" + sfx)(a.ref(), start, count)
            getattr(ref, "ref_insert_string" + sfx)(b.ref(), start, count)
            assert _same_tables(a, b), (kind, start, count)
        for pos in (62000, 62001, 62000, 62001, 12, 32768, 32769):
            got = getattr(oracle, "oracle_quick_insert_string" + sfx)(a.ref(), pos)
            want = getattr(ref, "ref_quick_insert_string" + sfx)(b.ref(), pos)
            assert got == want and _same_tables(a, b), (kind, pos)
    rng = np.random.default_rng(5)
    for h, v in rng.integers(0, 2**32, size=(2000, 2), dtype=np.uint64).tolist():
        assert oracle.oracle_update_hash(h, v) == ref.ref_update_hash(h, v)
        assert oracle.oracle_update_hash_roll(h, v) == ref.ref_update_hash_roll(h, v)


def test_compare256(oracle, ref):
    rng = np.random.default_rng(6)
    a = rng.integers(0, 2, size=4096, dtype=np.uint8)
    b = a.copy()
    b[rng.integers(0, 4096, size=24)] ^= 1
    for off in range(0, 4096 - 256, 13):
        assert oracle.oracle_compare256(a.ctypes.data + off, b.ctypes.data + off) == \
            ref.ref_compare256(a.ctypes.data + off, b.ctypes.data + off)


def _copy_cases():
    rng = np.random.default_rng(9)
    lens = list(range(1, 40)) + [63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 259, 511, 1000, 2047, 2048, 2049, 5000]
    cases = []
    for dist in list(range(1, 65)) + [255, 256, 257, 32768]:          # from behind out
        for ln in lens:
            cases.append((dist, ln, ln + int(rng.integers(0, 40))))
        cases += [(dist, 100, 60), (dist, 258, 1), (dist, 20, 7), (dist, 5000, 4999), (dist, 9, 8)]   # left < len
    for ahead in range(1, 301):                                        # from ahead of out, overlapping and not
        for ln in sorted({1, ahead - 1, ahead, ahead + 1, 2 * ahead + 3, 258, int(rng.integers(1, 5001))} - {0}):
            cases.append((-ahead, ln, ln + int(rng.integers(0, 40))))
        if ahead < 20 or ahead in (63, 64, 65, 255, 256, 257, 300):
            for ln in (2, 7, 8, 9, 15, 16, 17, 31, 100, 511, 512, 513, 1000, 2049, 5000):
                cases.append((-ahead, ln, ln + int(rng.integers(0, 40))))
            cases += [(-ahead, 300, 100), (-ahead, 5000, 4000), (-ahead, 12, 5)]
    return cases


def test_chunkmemset_safe(oracle, ref):
    """Only the contractual range [out, out + min(len, left)) and the returned pointer are compared: the reference's
    chunk stores may write beyond out + len (seen at dist 13, len 6, left 44), so each side works on its own copy."""
    rng = np.random.default_rng(10)
    room = 32768 + 5000 + 64
    base = rng.integers(0, 256, size=room + 8 + 5400, dtype=np.uint8)
    for phase in range(8):                                             # every alignment of out the reference treats apart
        for dist, ln, left in _copy_cases()[phase::8]:
            out = 32768 + 8 + phase
            a, b = base.copy(), base.copy()
            n = min(ln, left)
            end_a = oracle.oracle_chunkmemset_safe(a.ctypes.data + out, a.ctypes.data + out - dist, ln, left)
            end_b = ref.ref_chunkmemset_safe(b.ctypes.data + out, b.ctypes.data + out - dist, ln, left)
            assert end_a - a.ctypes.data == end_b - b.ctypes.data == out + n, (dist, ln, left)
            assert (a[out:out + n] == b[out:out + n]).all(), (dist, ln, left, phase)
            assert (a[:out] == base[:out]).all() and (b[:out] == base[:out]).all(), (dist, ln, left, phase)
