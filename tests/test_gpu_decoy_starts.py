"""Valid streams full of decoy block starts (tests/decoy_cases.py) through every large inflater of the device.  Every one of
them trusts a search for block starts and one safety net -- "a candidate that was noise is never reached", "anything
irregular on the chain sends the call to the sequential decoder" -- and the rest of the suite feeds that machinery streams
whose false candidates are as rare as chance makes them.  Here they come by the thousand, in a valid stream: markers,
stored headers that chain to each other and onto (or one byte off) genuine starts, dynamic headers at every bit offset,
decoy parts that overflow their slot, and complete FINAL blocks of other text behind a marker (a chain that enters one
ends with status 1 and wrong bytes: the sequential fallback cannot mask that).

Every entry point: status 1, out_len and in_used exact, the bytes, nothing written behind them, the same again on a second
call (parts, passes and host bytes included).  Against the fallback's masking: a stream with at most kPartsUnthinned
candidates and no expanding decoy must stay on the device with parts >= genuine blocks (the oracle's trace) - 2 -- with
spacing 1 every genuine byte-aligned stored start survives thin_starts and a genuine part ends on the next one; the 2 are
starts within 16 bytes of the end -- and the stream with cap2 + 1 candidates must be declined, not degraded.  ONE narrowing
of that floor, for the two streams that hold other blocks than the carrier's ("text", "steep"): a stored block that begins
off a byte boundary or is empty -- what a flush writes behind Huffman data -- is looked for by no finder (the stored pattern
is a byte pattern and wants LEN != 0, F1 takes BTYPE = 2 alone), so unless 00 00 ff ff ends where it begins it cannot be a
part of its own, and those blocks (decoy_cases.Stream.unfindable: 2 of 28 in "text", 2 of 11 in "steep", 0 elsewhere)
come off the count.  Every dynamic block stays on it: F2 walks inflate's own header rules, so it refuses no valid header.  What the decoys cost (parts, scratch, time) is measured by tools/decoy_starts_rate.py, not asserted here."""
import importlib
import zlib

import numpy as np
import pytest

import decoy_cases as dcy
import synth
import wrapped_members as wm
from test_gpu_inflate_index import Stream, read_check

pytestmark = pytest.mark.gpu

MiB = 1 << 20
FILL, GUARD = 0xA5, 4096
# at most kPartsUnthinned pattern candidates, no expanding decoy: the device path must do these itself
STAYS = ("c63", "c64", "chains", "dense", "steep", "text", "unthinned")
SMALL_FIRST = dcy.SMALL + dcy.LARGE


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), zr, importlib.import_module("zlib-ng_amd.oneshot")


def _dev(torch, data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _room(torch, n):
    return torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")


def _err(zr):
    return zr.rocm.lib().zng_rocm_last_error().decode()


def _mark(mods):
    """zng_rocm_last_error() keeps its text until the next one is set: a tiny stream through the large call leaves "stream
    below 128 KiB" there, so what a later call says is that call's own"""
    torch, inf, zr, _ = mods
    assert inf.inflate_large_dev(_dev(torch, b"\x03\x00"), torch.zeros(16, dtype=torch.uint8, device="cuda"))[:3] == (1, 0, 2)
    assert "below 128 KiB" in _err(zr)


def _why(zr):
    """why the call under test left the device path ("" when it said nothing: see _mark)"""
    text = _err(zr)
    return "" if "below 128 KiB" in text else text


def _bytes_are(dst, plain, note=""):
    got = dst.cpu().numpy()
    n = len(plain)
    assert got[:n].tobytes() == plain, ("bytes differ", note)
    assert bool((got[n:] == FILL).all()), ("written behind the end", note)


def _floor(s):
    """the parts a chain over the genuine starts has at least: a part per genuine block of the oracle's trace, less 2 for
    starts within 16 bytes of the end, less the stored blocks no finder looks for (the module's docstring)"""
    return len(s.genuine) - 2 - s.unfindable


def _gzip(raw, plain):
    return bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3]) + raw + wm.trailer(2, plain)


def _wrap(fmt, s):
    return b"\x78\x9c" + s.comp + wm.trailer(1, s.plain) if fmt == 1 else _gzip(s.comp, s.plain)


# ---- one stream: zng_rocm_inflate_large_dev / _ex_dev --------------------------------------------------------------------------
@pytest.mark.parametrize("subblock", [False, True])
@pytest.mark.parametrize("name", SMALL_FIRST)
def test_large_dev(mods, name, subblock):
    torch, inf, zr, _ = mods
    s = dcy.get(name)
    src = _dev(torch, s.comp)
    seen = []
    for _ in range(2):
        dst = _room(torch, len(s.plain))
        _mark(mods)
        st, n, used, parts = inf.inflate_large_dev(src, dst, subblock=subblock)
        why = _why(zr)
        print("decoys large_dev %s subblock=%d: parts %d (%s)" % (name, subblock, parts, why))
        assert (st, n, used) == (1, len(s.plain), len(s.comp)), (st, n, used, parts, why)
        _bytes_are(dst, s.plain, name)
        seen.append((st, n, used, parts))
        if name in STAYS:
            assert parts >= _floor(s), (parts, _floor(s), why)
        if name == "cap2+1":
            assert parts == 0 and "far more valid block headers" in why, (parts, why)
        if name == "dense-wide":
            assert parts == 0 and "far more" in why, (parts, why)
    assert seen[0] == seen[1]


# ---- pieces: zng_rocm_inflate_large_pieces_dev ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", STAYS[:-1] + ("expanding", "cut-short") + dcy.LARGE)
def test_pieces(mods, name):
    """a piece's slack is bounded by the piece, so here the decoys' promises (65280 bytes each in a dense run) overflow their
    slots and put "dense", "steep" and "cut-short" over the piece's retry cap.  No chain reaches them, so the piece must
    stay: the full parts ON its chain run again one at a time -- in "dense" the genuine stored parts that a decoy close
    behind their header cuts short, in "steep" a genuine block of 159 symbols per byte as well.  "cut-short" has 25 such
    parts, more than the kChainRetryTurns = 16 reruns a pass allows: it may leave the device, and must still be right."""
    torch, inf, zr, _ = mods
    s = dcy.get(name)
    piece = 4 * MiB
    if name in dcy.LARGE:                                 # the border between the two pieces lies among the decoys
        lo, hi = s.region
        near = [at for v in s.kinds.values() for at in v if abs(at - piece) < 4096]
        assert lo < piece < hi and near
    src = _dev(torch, s.comp)
    seen = []
    for _ in range(2):
        dst = _room(torch, len(s.plain))
        _mark(mods)
        st, n, used, parts, passes, host = inf.inflate_large_pieces_dev(src, dst, piece_bytes=piece)
        why = _why(zr)
        print("decoys pieces %s: parts %d passes %d host %d (%s)" % (name, parts, passes, host, why))
        assert (st, n, used) == (1, len(s.plain), len(s.comp)), (st, n, used, parts, passes, host, why)
        _bytes_are(dst, s.plain, name)
        seen.append((st, n, used, parts, passes, host))
        if name in STAYS:
            assert host == 0 and parts >= _floor(s), (host, parts, _floor(s), why)
    assert seen[0] == seen[1]


# ---- a batch: zng_rocm_inflate_large_streams_dev -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def neighbours():
    """benign streams: two stored carriers without a decoy, level-6 text, level-6 text with sync markers"""
    text = synth.silesia_like(3 * MiB // 2, seed=0xBE9).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    flushed = b"".join(c.compress(text[k:k + 65536]) + c.flush(zlib.Z_SYNC_FLUSH) for k in range(0, len(text), 65536)) + c.flush()
    a, b = dcy.benign(256 << 10, 1), dcy.benign(700 << 10, 2)
    return [(a.comp, a.plain), (wm.raw(text), text), (b.comp, b.plain), (flushed, text)]


@pytest.mark.parametrize("subblock", [False, True])
def test_streams_batch_and_its_neighbours(mods, neighbours, subblock):
    torch, inf, zr, _ = mods
    decoys = [dcy.get(k) for k in ("c64", "dense-wide", "expanding", "unthinned", "cap2+1")]

    def run(streams, round_bytes=0):
        srcs = [_dev(torch, c) for c, _ in streams]
        dsts = [_room(torch, len(p)) for _, p in streams]
        rc, rows, rounds, launches = inf.inflate_large_streams_dev(srcs, dsts, round_bytes=round_bytes, subblock=subblock)
        assert rc == 0, (rc, _err(zr))
        for k, ((c, p), d, r) in enumerate(zip(streams, dsts, rows)):
            assert r[:4] == (1, len(p), len(c), None), (k, r, _err(zr))
            _bytes_are(d, p, k)
        return rows, rounds

    alone, _ = run(neighbours)
    assert all(r[4] >= 4 for r in alone), alone           # the benign streams are the device's
    # interleaved: neighbour, decoy, neighbour, decoy, ...
    mixed, where = [], []
    for k, s in enumerate(decoys):
        if k < len(neighbours):
            where.append(len(mixed))
            mixed.append(neighbours[k])
        mixed.append((s.comp, s.plain))
    assert len(where) == len(neighbours)
    for round_bytes in (0, 4 * MiB):                      # 4 MiB: rounds end between them
        rows, rounds = run(mixed, round_bytes)
        print("decoys batch subblock=%d round_bytes=%d: rounds %d rows %s" % (subblock, round_bytes, rounds, [r[4:] for r in rows]))
        assert rounds >= (3 if round_bytes else 1)
        got = [rows[w] for w in where]
        if subblock:
            # (SUBBLOCK places sub-starts with a step and a "split dynamic blocks" decision that are the PASS's -- pass_run: the
            # heavy parts of all its streams against the chip's slots -- so a neighbour's sub-parts depend on the company it
            # keeps, whoever that is; what must hold is that it stays the device's)
            assert [r[:4] for r in got] == [r[:4] for r in alone] and all(r[4] >= 4 for r in got), (round_bytes, got, alone, _err(zr))
        else:
            assert got == alone, (round_bytes, got, alone, _err(zr))
        again, _ = run(mixed, round_bytes)
        assert [r[:4] for r in again] == [r[:4] for r in rows]


# ---- wrapped: zng_rocm_uncompress_large_dev / _streams_dev --------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 2])
def test_wrapped(mods, fmt):
    torch, inf, zr, _ = mods
    three = [dcy.get(k) for k in ("chains", "expanding", "first+1")]
    members = [_wrap(fmt, s) for s in three]
    for s, m in zip(three, members):                      # (CPython reads them: the wrappers are sound)
        assert zlib.decompress(m, 15 if fmt == 1 else 31) == s.plain
        src = wm.place(torch, m, 3)
        for _ in range(2):
            dst = _room(torch, len(s.plain))
            st, n, used, parts, passes, host = inf.uncompress_large_dev(fmt, src, dst, piece_bytes=4 * MiB)
            assert (st, n, used) == (1, len(s.plain), len(m)), (s.name, st, n, used, parts, passes, host, _err(zr))
            _bytes_are(dst, s.plain, s.name)
    srcs = [wm.place(torch, m, wm.ODDS[k]) for k, m in enumerate(members)]
    for _ in range(2):
        dsts = [_room(torch, len(s.plain)) for s in three]
        rc, rows, rounds, launches = inf.uncompress_large_streams_dev(fmt, srcs, dsts)
        assert rc == 0, (rc, _err(zr))
        for s, m, d, r in zip(three, members, dsts, rows):
            assert r[:4] == (1, len(s.plain), len(m), None), (s.name, r, _err(zr))
            _bytes_are(d, s.plain, s.name)


# ---- the counting pass: zng_rocm_uncompress_large_size_dev / _sizes_dev ----------------------------------------------------------
def test_sizes(mods):
    torch, inf, zr, _ = mods
    all_ = [dcy.get(k) for k in SMALL_FIRST]
    srcs = [_dev(torch, s.comp) for s in all_]
    for s, src in zip(all_, srcs):
        for _ in range(2):
            st, n, used, parts = inf.uncompress_large_size_dev(0, src)
            print("decoys size %s: parts %d" % (s.name, parts))
            assert (st, n, used) == (1, len(s.plain), len(s.comp)), (s.name, st, n, used, parts, _err(zr))
    for round_bytes in (0, 4 * MiB):
        rc, rows, rounds, launches = inf.uncompress_large_sizes_dev(0, srcs, round_bytes=round_bytes)
        assert rc == 0, (rc, _err(zr))
        assert [r[:4] for r in rows] == [(1, len(s.plain), len(s.comp), None) for s in all_], (rows, _err(zr))
    # wrapped: the trailer's ISIZE / the member's end are checked against the count
    for fmt in (1, 2):
        for s in (dcy.get("chains"), dcy.get("first+1")):
            m = _wrap(fmt, s)
            st, n, used, parts = inf.uncompress_large_size_dev(fmt, wm.place(torch, m, 5))
            assert (st, n, used) == (1, len(s.plain), len(m)), (fmt, s.name, st, n, used, _err(zr))


# ---- every member of a gzip file: zng_rocm_gunzip_members_dev ---------------------------------------------------------------------
@pytest.mark.parametrize("subblock", [False, True])
def test_gunzip_members(mods, subblock):
    torch, inf, zr, _ = mods
    four = [dcy.get(k) for k in ("c64", "chains", "dense", "expanding")]
    members = [_gzip(s.comp, s.plain) for s in four]
    data, plain = b"".join(members), b"".join(s.plain for s in four)
    want, at, out = [], 0, 0
    for s, m in zip(four, members):
        want.append((at, len(m), out, len(s.plain), zlib.crc32(s.plain), 0))
        at, out = at + len(m), out + len(s.plain)
    src = wm.place(torch, data, 7)
    for _ in range(2):
        dst = _room(torch, len(plain))
        st, n, used, rows, nmembers, counters = inf.gunzip_members_dev(src, dst, subblock=subblock)
        assert (st, n, used, nmembers) == (1, len(plain), len(data), 4), (st, n, used, nmembers, counters, _err(zr))
        assert rows == want, (rows, want)
        _bytes_are(dst, plain)


# ---- random access: zng_rocm_inflate_index_build_dev / _read_dev ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chains", "text", "unthinned"])
def test_index_points_and_reads(mods, name):
    torch, inf, zr, _ = mods
    s = dcy.get(name)
    stream = Stream(mods, s.comp, s.plain, 0, odd=5)
    st, out_len, in_used, idx, dst, counters, why = stream.build(span=64 << 10, piece_bytes=4 * MiB)
    assert (st, out_len, in_used) == (1, len(s.plain), len(s.comp)) and idx is not None, (st, out_len, in_used, counters, why)
    assert dst[:out_len].cpu().numpy().tobytes() == s.plain
    pts = idx.points()
    genuine = set(s.genuine)
    assert len(pts) >= 3 and all(in_bit in genuine for in_bit, _, _ in pts), [p for p in pts if p[0] not in genuine][:5]
    assert idx.plain_len == len(s.plain)
    # 50 ranges: seeded, inside the decoy region, across every shadow and the chains' ends
    rng = np.random.default_rng(0x1DEC)
    ranges = [(int(rng.integers(0, len(s.plain))), int(rng.integers(1, 70000)), k % 16) for k in range(30)]
    first = s.plain.find(dcy.MARKER)
    assert first >= 0
    ranges += [(first + int(rng.integers(0, 100000)), int(rng.integers(1, 5000)), k % 16) for k in range(12)]
    for at, text in s.shadows:
        off = s.plain.find(dcy.shadow_block(text))
        assert off >= 0
        ranges += [(off - 100, len(text) + 300, 3), (off + 4, 64, 0)]
    for kind in ("chain-on", "chain-off"):
        last, to = s.lands[kind]
        off = s.plain.find(s.comp[last - 54:last + 5])
        assert off >= 0
        ranges += [(off, 400, 1), (off + 50, 70000, 9)]
    assert len(ranges) >= 50
    read_check(mods, idx, stream.src, s.plain, ranges)
    read_check(mods, idx, stream.src, s.plain, ranges)
    idx.close()


# ---- the streaming hook's blocks mode, and the host-resident one-shots --------------------------------------------------------------
def test_hook_blocks_on_a_piece_cut_inside_a_decoy(mods):
    torch, inf, zr, _ = mods
    s = dcy.get("unthinned")
    cut = max(at for at in s.kinds["marker"] if at < 5 * MiB) + 2          # between the two halves of a marker
    assert cut >= 4 * MiB
    want_end = max(b for b in s.genuine if b <= 8 * cut)
    hook = inf.InflateHook()
    try:
        for _ in range(2):
            st, out, end_bit, cv, msg = hook.inflate_blocks(s.comp[:cut], check=2)
            assert (st, end_bit, msg) == (0, want_end, ""), (st, end_bit, want_end, msg, _err(zr))
            # the plaintext in front of that block: the stored carrier's payloads up to it
            n = len(zlib.decompressobj(-15).decompress(s.comp[:want_end // 8] + b"\x01\x00\x00\xff\xff"))
            assert out == s.plain[:n] and cv == zlib.crc32(out)
            assert zr.lib().zng_rocm_inflate_large_last_parts() >= sum(1 for b in s.genuine if b < want_end) - 2, _err(zr)
    finally:
        hook.close()


@pytest.mark.parametrize("name", ["chains", "expanding", "unthinned", "cap2+1"])
def test_host_resident_one_shots(mods, name):
    torch, inf, zr, _ = mods
    s = dcy.get(name)
    for _ in range(2):
        dst = _room(torch, len(s.plain))
        rc, n = inf.inflate_raw(s.comp, dst)
        assert (rc, n) == (1, len(s.plain)), (rc, n, _err(zr))
        _bytes_are(dst, s.plain, name)
        dst = _room(torch, len(s.plain))
        out = inf.inflate_raw_threads(s.comp, dst, nthreads=8)
        assert out == (1, len(s.plain), len(s.comp)), (out, _err(zr))
        _bytes_are(dst, s.plain, name)
