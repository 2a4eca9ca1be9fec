"""CPU: the decoy streams of tests/decoy_cases.py are what they claim to be -- valid, with the intended number of places that
pass the finders' byte patterns, every decoy kind present and decodable as its docstring says -- and the host decoders
(one thread, eight threads, blocks mode) read them like any other stream.  The device side: tests/test_gpu_decoy_starts.py."""
import zlib

import numpy as np
import pytest

import decoy_cases as dcy
import inflate_util
from test_inflate_threads_cpu import _check, env  # noqa: F401  (the fixture and the one-thread / eight-thread comparison)

_HEADER_ERRORS = {"invalid block type", "invalid stored block lengths", "too many length or distance symbols",
                  "invalid code lengths set", "invalid bit length repeat", "invalid code -- missing end-of-block",
                  "invalid literal/lengths set", "invalid distances set"}


def _from_bit(comp, bit, nbytes):
    """the stream from bit `bit` on, moved to bit 0"""
    lo = bit >> 3
    v = int.from_bytes(comp[lo:lo + nbytes + 1], "little") >> (bit & 7)
    return v.to_bytes(nbytes + 1, "little")[:nbytes]


@pytest.mark.parametrize("name", dcy.ALL)
def test_streams_are_valid_and_counted(name):
    s = dcy.get(name)
    z = zlib.decompressobj(-15)
    assert z.decompress(s.comp) == s.plain and z.eof and not z.unused_data
    st, msg, out, used = inflate_util.oracle_inflate(s.comp, cap=len(s.plain) + 64)
    assert (st, used) == (1, len(s.comp)) and out == s.plain, (st, msg, used)
    # the genuine blocks: the stored carrier's are byte-aligned and every one but the stream's first passes the stored pattern
    m, sp = dcy.pattern_candidates(s.comp)
    lo, hi = s.region
    carrier = [b for b in s.genuine if 8 * lo < b < 8 * hi]
    assert all(b % 8 == 0 for b in carrier) and set(b // 8 for b in carrier) <= set(sp.tolist())
    assert s.count == len(m) + len(sp)
    assert dcy.MIN_LARGE <= len(s.comp) <= (9 << 20)
    assert s.retry_bound <= dcy.RETRY_LIMIT
    if name in dcy.LARGE:
        assert s.count == dcy.large_cell(name, len(s.comp))
        assert len(s.comp) > (6 << 20) and dcy.patterns_first(len(s.comp)) < dcy.cap2(len(s.comp))
    elif name in ("c63", "c64"):
        assert s.count == int(name[1:])
    elif name == "dense-wide":
        assert s.count > 4 * dcy.cap2(len(s.comp))
    else:
        assert 40 <= s.count <= dcy.PARTS_UNTHINNED


def test_the_count_cells_are_the_plans_bounds():
    n = len(dcy.large("first").comp)
    cells = sorted([63, 64] + [dcy.large_cell(k, n) for k in dcy.LARGE])
    assert cells == [63, 64, 12288, 12289, 16384, 16385, n // 512 + 4096, n // 512 + 4097]
    # one carrier: the large cells differ in their markers alone
    a, b = dcy.large("unthinned"), dcy.large("cap2+1")
    assert len(a.comp) == len(b.comp) and a.genuine == b.genuine
    for kind in ("stored-chain", "stored-far", "dynamic", "shadow", "chain-on", "chain-off"):
        assert a.kinds[kind] == b.kinds[kind]


def test_every_kind_is_present_and_is_what_it_says():
    seen = set()
    for name in dcy.ALL:
        seen |= set(dcy.get(name).kinds)
    assert seen == {"marker", "marker-dense", "stored-chain", "stored-far", "dynamic", "expanding", "shadow", "chain-on", "chain-off"}
    for name in dcy.ALL:
        s = dcy.get(name)
        m, sp = dcy.pattern_candidates(s.comp)
        markers, stored, genuine = set(m.tolist()), set(sp.tolist()), set(s.genuine)
        for at in s.kinds.get("marker", []):
            assert at in markers and 8 * (at + 4) not in genuine
        for at in s.kinds.get("stored-far", []):
            ln = int.from_bytes(s.comp[at + 1:at + 3], "little")
            assert at in stored and 8 * at not in genuine and at + 5 + ln <= len(s.comp) - 64
        for at in s.kinds.get("stored-chain", []):        # every header lands on the next one
            n, b = 0, at
            while b in stored and s.comp[b + 1:b + 3] == b"\x01\x00" and b + 6 in stored:
                n, b = n + 1, b + 6
            assert n + 1 in (2, 10, 1000), (name, at, n)
        for at in s.kinds.get("marker-dense", []):
            reps = 12000 if name == "dense-wide" else 1000
            inside = [b for b in range(at, at + 4 * reps - 8)]
            assert sum(b in markers for b in inside) >= reps - 2 and sum(b in stored for b in inside) >= 2 * reps - 6
            if name == "dense-wide":
                # one 4096-byte scan step of the table finder (its items begin at multiples of 4096 bytes of the stream) that
                # lies inside the run: more candidates than the workgroup's list holds (kFindLocal = 2048)
                base = (at + 4095) & ~4095
                assert base + 4096 <= at + 4 * reps
                step = sum(base <= b < base + 4096 for b in markers) + sum(base <= b < base + 4096 for b in stored)
                assert step > 2048, step
        for kind, off in (("chain-on", 0), ("chain-off", 1)):
            if kind in s.lands:
                last, to = s.lands[kind]
                ln = int.from_bytes(s.comp[last + 1:last + 3], "little")
                assert last in stored and last + 5 + ln == to
                assert (8 * to in genuine) == (off == 0) and 8 * (to + off) in genuine
        # shadow: decoded on its own from the bit behind its marker, a complete stream of other text
        for at, text in s.shadows:
            bit = 8 * (at + 4)
            assert at in markers and bit not in genuine
            st, msg, out, used = inflate_util.oracle_inflate(_from_bit(s.comp, bit, len(text) * 2 + 16), cap=len(text) + 64)
            assert (st, out) == (1, text) and text not in s.plain, (name, at, st, msg)
        # expanding: more than kSlotRatio symbols per byte AND more than the slot's slack; it ends on another marker
        for at, produced in s.expanding:
            bit = 8 * (at + 4)
            bits = dcy.candidate_bits(s.comp)
            nxt = int(bits[np.searchsorted(bits, bit, side="right")])
            part_bytes = (nxt - bit + 7) >> 3
            assert produced > part_bytes * dcy.SLOT_RATIO + dcy.SLOT_SLACK, (name, at, produced, part_bytes)
            assert s.comp[(nxt >> 3) - 4:nxt >> 3] == dcy.MARKER
            # the part's own blocks: the fixed block, the empty stored block, and it stops on the next marker's bit
            piece = _from_bit(s.comp, bit, part_bytes) + dcy._stored(b"", True)
            st, msg, out, used = inflate_util.oracle_inflate(piece, cap=produced + 64)
            assert (st, len(out), used) == (1, produced, len(piece)), (name, at, st, msg, len(out), used)
        # dynamic: the header is accepted at the bit it was put on.  What follows is filler, so the decoder fails later: in the
        # block's codes, or -- the block has ended -- somewhere in a second block
        for at, k in s.dynamics:
            piece = _from_bit(s.comp, 8 * at + k, 400)
            assert piece[0] & 7 == 4                      # BFINAL 0, BTYPE 2
            st, blocks = inflate_util.oracle_block_starts(piece, 1 << 16)
            msg = inflate_util.oracle_inflate(piece, cap=1 << 16)[1]
            assert len(blocks) >= 2 or msg not in _HEADER_ERRORS, (name, at, k, msg)
        if name == "chains":
            assert {k for _, k in s.dynamics} == set(range(8)) and len(s.dynamics) == 8 * len(dcy.dynamic_headers()) + 18


@pytest.mark.parametrize("name", dcy.ALL)
def test_host_decoders(env, name):
    zr, inf = env
    s = dcy.get(name)
    _check(env, s.comp, s.plain)
    # blocks mode from bit 0: the whole stream, and a prefix cut inside the decoy region -- complete genuine blocks only
    whole = inf.decode_blocks(s.comp)
    assert (whole.status, whole.end_bit, whole.out_len) == (1, 8 * len(s.comp), len(s.plain))
    lo, hi = s.region
    cut = dcy.cut_inside_a_decoy(s)
    assert lo < cut < hi
    part = inf.decode_blocks(s.comp[:cut])
    assert part.status == 0 and part.end_bit == max(b for b in s.genuine if b <= 8 * cut)
    # ... and their plaintext: what CPython makes of the stream up to that block start, closed by an empty final block
    assert part.end_bit % 8 == 0 and (part.end_bit > 0 or name == "dense-wide")
    assert part.out_len == len(zlib.decompressobj(-15).decompress(s.comp[:part.end_bit // 8] + dcy._stored(b"", True)))
