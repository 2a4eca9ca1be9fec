"""Crafted stored blocks (tests/stored_cases.py) through every device decoder.  What each restates is the stored block of
inflate.c:759-800:
  the stream kernel (inflate_streams_body.h: the payload copy in pieces through the ring, the flush inside the piece loop, LEN /
      NLEN out of the bit buffer, the seek behind the payload) -- every valid case on its own, every bad NLEN, every cut of the
      input and every room that ends in or behind the payload;
  the sizing kernel (inflate_sizes_body.h) -- the same blobs, its rows against the decoder's and the oracle's;
  the dictionary-object form -- the cases whose copies reach into history;
  part mode in both LDS layouts, the sub-start parse and the counting kernels (inflate_large.hip, inflate_large_size.hip) -- ONE
      stream of groups around stored blocks, behind markers and without;
  the span form (random access) -- ranges that begin and end at the lane and piece borders of a stored payload.
Expected: the plaintext (replay() of the tokens plus the payloads, CPython's zlib for the large streams), the oracle for every
refusal and for what a cut stream still delivers.  No device output is ever the expected value."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import inflate_util
import stored_cases as sc
from gpu_common import torch_mod
from test_gpu_inflate_dev import _run, inf  # noqa: F401  (the fixture and the batch runner: it checks the bytes around every output)
from test_gpu_inflate_index import Stream, read_check
from test_gpu_inflate_sizes import _decode, _lay, _same, _sizes

pytestmark = pytest.mark.gpu
STARVED = "input ended before the final block"             # the message of test_truncated_input_and_small_output
FULL = "output buffer too small"
BAD_LEN = "invalid stored block lengths"
KiB = 1 << 10


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.inflate"), zr


def _dev(torch, data):
    return torch.from_numpy(np.frombuffer(bytes(data), dtype=np.uint8).copy()).cuda()


def _err(zr):
    return zr.rocm.lib().zng_rocm_last_error().decode()


# ---- 1: the stream kernel, valid streams ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sc.VALID)
def test_valid_cases_through_the_stream_kernel(inf, family):
    cases = sc.cases(family)
    for pad in (0, 1, 2, 3) if family == "window" else (0,):   # every lead of the stream's first word
        rows, outs = _run(inf, [c.stream for c in cases], [len(c.plain) for c in cases], dicts=[c.history for c in cases], pad_in=pad)
        for c, r, o in zip(cases, rows, outs):
            assert r == (1, len(c.plain), len(c.stream), ""), (pad, c.name, r)
            assert o == c.plain, (pad, c.name)


# ---- 2: the stream kernel, ends -------------------------------------------------------------------------------------------------
def test_bad_nlen_through_the_stream_kernel(inf):
    cases = sc.cases("nlen")
    rows, outs = _run(inf, [c.stream for c in cases], [4096] * len(cases))
    for c, r, o in zip(cases, rows, outs):
        ost, omsg, oout, _ = inflate_util.oracle_inflate(c.stream, 4096)
        assert (ost, omsg) == (-3, BAD_LEN)
        assert (r[0], r[3], r[1]) == (ost, omsg, len(oout)) and o == oout, (c.name, r)


def test_every_cut_through_the_stream_kernel(inf):
    cases = sc.cases("cuts")
    # with the room of the whole plaintext, and with room for exactly the bytes that are there (the oracle's answer is the same)
    for exact in (False, True):
        caps = [len(c.plain) if exact else c.meta["cap"] for c in cases]
        rows, outs = _run(inf, [c.stream for c in cases], caps)
        differ = []
        for c, cap, r, o in zip(cases, caps, rows, outs):
            ost, omsg, oout, _ = inflate_util.oracle_inflate(c.stream, cap)
            assert (ost, omsg, oout) == (-5, STARVED, c.plain)
            if (r[0], r[3], r[1]) != (-5, STARVED, len(oout)) or o != oout:     # every cut is compared: none is left undecided
                differ.append((c.name, cap, r, len(oout)))
        assert not differ, (exact, len(differ), differ[:5])


def test_room_through_the_stream_kernel(inf):
    runs = sc.room_runs()
    rows, outs = _run(inf, [r.case.stream for r in runs], [r.cap for r in runs], dicts=[r.case.history for r in runs])
    differ = []
    for run, r, o in zip(runs, rows, outs):
        c = run.case
        if run.exact:
            ok = r == (1, len(c.plain), len(c.stream), "") and o == c.plain
        else:
            ok = (r[0], r[3]) == (-5, FULL) and r[1] <= run.cap and o == c.plain[:r[1]]
        if not ok:
            differ.append((c.name, run.cap, r))
    assert not differ, (len(differ), differ[:5])
    assert sum(1 for run in runs if run.exact) > 100


# ---- 3: the sizing kernel -------------------------------------------------------------------------------------------------------
def test_sizing_kernel_over_the_same_blobs(inf):
    items = [(c, len(c.plain)) for c in sc.valid_cases()] + [(c, 4096) for c in sc.cases("nlen")] + \
        [(c, c.meta["cap"]) for c in sc.cases("cuts")]
    blobs, hist, caps = [c.stream for c, _ in items], [len(c.history) for c, _ in items], [cap for _, cap in items]
    laid = _lay(blobs)
    rows = _sizes(inf, blobs, 0, dict_len=hist, laid=laid)
    dec = _decode(inf, blobs, caps, dict_len=hist, laid=laid)
    differ = []
    for (c, cap), r, d in zip(items, rows, dec):
        if c.family == "nlen":
            ok = (r[0], r[3]) == (-3, BAD_LEN)
        elif c.family == "cuts":
            ok = (r[0], r[3], r[1]) == (-5, STARVED, len(c.plain))                # the oracle's partial length (the CPU file holds it to that)
        else:
            ok = r == (1, len(c.plain), len(c.stream), "")
        if not (ok and _same(r, d)):
            differ.append((c.name, r, d))
    assert not differ, (len(differ), differ[:5])


# ---- 4: the dictionary-object form ----------------------------------------------------------------------------------------------
def test_history_cases_through_the_dictionary_object(inf):
    torch = torch_mod()
    dfl = importlib.import_module("zlib-ng_amd.deflate")
    cases = [c for c in sc.cases("after") if c.meta["form"] == 3]
    assert len(cases) >= 50 and all(c.history == sc.HISTORY[-300:] for c in cases)
    in_off, pos = [], 1
    for c in cases:
        in_off.append(pos)
        pos += len(c.stream) + 3
    src = np.zeros(pos + 64, dtype=np.uint8)
    for o, c in zip(in_off, cases):
        src[o:o + len(c.stream)] = np.frombuffer(c.stream, dtype=np.uint8)
    out_off, pos = [], 5
    for c in cases:
        out_off.append(pos)
        pos += len(c.plain) + 7
    dst = torch.full((pos + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dic = dfl.Dictionary(sc.HISTORY[-300:])
    try:
        b = inf.InflateDevBatch(torch.from_numpy(src).cuda(), in_off, [len(c.stream) for c in cases], dst, out_off, [len(c.plain) for c in cases])
        b.run_dict(0, dic)
        rows = b.rows()
    finally:
        dic.close()
    got = dst.cpu().numpy()
    assert got[:5].tolist() == [0xA5] * 5
    for c, r, o in zip(cases, rows, out_off):
        assert r == (1, len(c.plain), len(c.stream), ""), (c.name, r)
        assert got[o:o + len(c.plain)].tobytes() == c.plain, c.name
        assert got[o + len(c.plain):o + len(c.plain) + 7].tolist() == [0xA5] * 7, c.name


# ---- 5, 6: part mode and the counting kernels -------------------------------------------------------------------------------------
def _cpython(big):
    z = zlib.decompressobj(-15, zdict=big.history) if big.history else zlib.decompressobj(-15)
    plain = z.decompress(big.comp)
    assert z.eof and not z.unused_data and plain == big.plain
    return plain


def _large(mods, big, subblock=False, min_parts=0):
    torch, inf, zr = mods
    plain = _cpython(big)
    dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(_dev(torch, big.comp), dst, window=_dev(torch, big.history) if big.history else None,
                                               subblock=subblock)
    assert (st, n, used) == (1, len(plain), len(big.comp)), (st, n, used, parts, _err(zr))
    assert parts >= min_parts, (parts, min_parts, _err(zr))
    assert dst[:n].cpu().numpy().tobytes() == plain
    assert int(dst[n:].max()) == 0                        # nothing written behind the end
    return parts


def _cus(zr):
    info = (4 * C.c_int32)()
    assert zr.rocm.lib().zng_rocm_device_info(info) == 0
    return int(info[0])


def test_part_mode_behind_markers(mods):
    big = sc.large_stream(True)
    assert len(big.comp) >= (128 << 10)
    print("parts, markers: %d of %d groups" % (_large(mods, big, min_parts=big.groups), big.groups))


def test_part_mode_sub_starts(mods):
    big = sc.large_stream(True)
    print("parts, markers, sub-starts: %d of %d groups" % (_large(mods, big, subblock=True, min_parts=big.groups), big.groups))


def test_part_mode_without_markers(mods):
    big = sc.large_stream(False)
    assert len(big.comp) >= (128 << 10)
    print("parts, no markers: %d (%d groups, %d blocks)" % (_large(mods, big), big.groups, big.blocks))    # reported, not asserted


def test_part_mode_with_a_window(mods):
    big = sc.large_stream(True, lead=False)
    assert len(big.history) == 32768 and len(big.comp) >= (128 << 10)
    print("parts, markers, 32 KiB window: %d of %d groups" % (_large(mods, big, min_parts=big.groups), big.groups))


def test_packed_part_layout(mods):
    torch, inf, zr = mods
    cus = _cus(zr)
    big = sc.large_stream(True, tiny=12 * cus + 200)
    assert big.groups >= 12 * cus + 200
    plain = _cpython(big)
    dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    piece = 4 << 20
    assert len(big.comp) < piece                          # ONE piece holds all the parts: their count is that launch's
    st, n, used, parts, passes, host = inf.inflate_large_pieces_dev(_dev(torch, big.comp), dst, piece_bytes=piece)
    assert passes == 1, passes
    assert (st, n, used, host) == (1, len(plain), len(big.comp), 0), (st, n, used, host, _err(zr))
    assert parts > 12 * cus, (parts, cus, _err(zr))
    assert dst[:n].cpu().numpy().tobytes() == plain and int(dst[n:].max()) == 0
    print("parts, %d tiny groups in one piece: %d" % (big.groups, parts))


def test_counting_kernels(mods):
    torch, inf, zr = mods
    for big in (sc.large_stream(True), sc.large_stream(False), sc.large_stream(True, lead=False),
                sc.large_stream(True, tiny=12 * _cus(zr) + 200)):
        st, n, used, parts = inf.uncompress_large_size_dev(0, _dev(torch, big.comp), dict_len=len(big.history))
        assert (st, n, used) == (1, len(big.plain), len(big.comp)), (st, n, used, parts, _err(zr))


# ---- 7: the span form -----------------------------------------------------------------------------------------------------------
def test_spans_that_begin_and_end_inside_stored_payloads(mods):
    torch, inf, zr = mods
    big = sc.large_stream(True)
    s = Stream((torch, inf, zr, None), big.comp, _cpython(big), 0)
    st, out_len, in_used, idx, dst, counters, err = s.build(span=64 * KiB)
    assert (st, out_len, in_used) == (1, len(big.plain), len(big.comp)), (st, out_len, in_used, err)
    assert dst[:out_len].cpu().numpy().tobytes() == big.plain and idx is not None and len(idx.points()) >= 3
    ranges, k = [], 0
    for rec in big.stored:
        if rec.length not in (48, 49, 513, 1025, 4097, 65535):
            continue
        a, L = rec.out_at, rec.length
        edges = sorted({a + d for d in (0, 1, 15, 16, 17)} | {a + L - d for d in (0, 1, 15, 16, 17)})
        assert big.plain[a:a + L] == big.comp[rec.in_at:rec.in_at + L]
        for b in edges:
            for e in edges + [a + L + 100]:               # ... and one end in the block behind the payload
                if b < e:
                    ranges.append((b, e - b, k % 16))
                    k += 1
        ranges += [(a - 100, e - (a - 100), (k + j) % 16) for j, e in enumerate(edges)]    # from the block in front into the payload
    assert len(ranges) > 300
    counters = read_check((torch,), idx, s.src, big.plain, ranges)
    assert counters["decoded"] > 0 and counters["rounds"] >= 1
