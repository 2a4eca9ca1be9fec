"""Crafted dynamic-Huffman blocks (tests/dynamic_cases.py) through every device decoder.  What each restates is the dynamic
header of inflate.c:814-917 and the table construction of inftrees.c:32-297:
  the stream kernel (inflate_dev.hip: build_code / long_code at roots 10 / 9, the hand-written decode loop and its exits to
      the long-code path) -- every case on its own, with room and without, every invalid block, every truncation;
  part mode (roots 10 / 8; inflate_large.hip) -- ONE stream of all the cases, each behind a sync marker;
  the block-start finder (F1's masks and Kraft test, validate_one's second header walk) -- the same blocks with no marker,
      each at whatever bit the one in front ended on, every kind of header on its share of them;
  the sub-start parse (lane_long_code, the dry parse of subblock_sync_kernel) -- long blocks of the deep code sets;
  the packed part layout (InflateLdsPart: code-length tables in the distance table's place, 16-bit first / offs) -- more
      parts than 12 per CU.
Expected: the plaintext (replay() of the tokens, CPython's zlib for the large streams), the oracle for every refusal."""
import ctypes as C
import importlib
import zlib

import numpy as np
import pytest

import dynamic_cases as dc
import inflate_util
from test_gpu_inflate_dev import _run, inf  # noqa: F401  (the fixture and the batch runner)

pytestmark = pytest.mark.gpu


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


def _cpython(comp, window=b""):
    z = zlib.decompressobj(-15, zdict=window) if window else zlib.decompressobj(-15)
    plain = z.decompress(comp)
    assert z.eof and not z.unused_data
    return plain


# ---- 1 / 2: the stream kernel -----------------------------------------------------------------------------------------------
def test_every_valid_case_through_the_stream_kernel(inf):
    cases = dc.valid_cases()
    streams, plains, dicts = [c.stream for c in cases], [c.plain for c in cases], [c.history for c in cases]
    rows, outs = _run(inf, streams, [len(p) for p in plains], dicts=dicts)      # (_run checks the bytes around every output)
    for c, r, o in zip(cases, rows, outs):
        assert r == (1, len(c.plain), len(c.stream), ""), (c.name, r)
        assert o == c.plain, c.name
    # the long code at the refetch, with every lead of the stream's first word
    refill = [c for c in cases if c.kind == "refill"]
    assert len(refill) == 128
    for pad in (1, 2, 3):
        rows, outs = _run(inf, [c.stream for c in refill], [len(c.plain) for c in refill], dicts=[c.history for c in refill],
                          pad_in=pad)
        for c, r, o in zip(refill, rows, outs):
            assert r == (1, len(c.plain), len(c.stream), "") and o == c.plain, (pad, c.name, r)
    # room that ends inside the output: the reference's status, and a prefix of the plaintext
    some = [c for c in cases if len(c.plain) > 0]
    short = [max(0, len(c.plain) - 1 - k % 70) for k, c in enumerate(some)]
    rows, outs = _run(inf, [c.stream for c in some], short, dicts=[c.history for c in some])
    for c, cap, r, o in zip(some, short, rows, outs):
        assert r[0] == -5 and r[3] == "output buffer too small", (c.name, r)
        assert r[1] <= cap and o == c.plain[:r[1]], c.name


def test_every_refusal_and_truncation_through_the_stream_kernel(inf):
    inv = dc.invalid_cases()
    items = [(x.name, x.stream, x.expect) for x in inv] + [("sweep", s, e) for s, e in dc.truncation_sweep()]
    rows, outs = _run(inf, [s for _, s, _ in items], [dc.CAP] * len(items))
    differ, undecided = [], 0
    for (name, s, (ost, omsg, oout, oused)), r, o in zip(items, rows, outs):
        if ost == -5 and r[0] == -5:
            undecided += 1                                # both out of input: the partial output is not compared
            continue
        if (r[0], r[3]) != (ost, omsg) or (ost == 1 and (o != oout or r[2] != oused)):
            differ.append((name, s.hex(), r, (ost, omsg, oused)))
    assert not differ, (len(differ), differ[:5])
    # (the oracle alone leaves less than 60 % of the sweep and none of the invalid list undecided:
    # tests/test_inflate_dynamic_cpu.py, test_the_sweep_is_mostly_decided)
    assert undecided < 0.6 * (len(items) - len(inv))


# ---- 3 .. 5: part mode --------------------------------------------------------------------------------------------------------
def _large(mods, big, subblock=False, window=b"", min_parts=0):
    torch, inf, zr = mods
    plain = _cpython(big.comp, window)
    src = _dev(torch, big.comp)
    dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(src, dst, window=_dev(torch, window) if window else None, subblock=subblock)
    assert (st, n, used) == (1, len(plain), len(big.comp)), (st, n, used, parts, _err(zr))
    assert parts >= min_parts, (parts, min_parts, _err(zr))
    assert dst[:n].cpu().numpy().tobytes() == plain
    assert int(dst[n:].max()) == 0                        # nothing written behind the end
    return parts


def test_part_mode_behind_markers(mods):
    big = dc.large_stream(True)
    assert len(big.comp) >= (128 << 10) and set(big.share) == set(dc.kinds())
    _large(mods, big, min_parts=big.blocks)
    # no noise in front: the first parts' copies reach into the window
    first = dc.large_stream(True, lead=False)
    _large(mods, first, window=dc.HISTORY, min_parts=first.blocks)


def test_part_mode_block_starts_are_found(mods):
    big = dc.large_stream(False)
    assert len(big.comp) >= (128 << 10) and set(big.share) == set(dc.kinds())
    assert min(big.share.values()) >= 0.05, big.share
    status, blocks = inflate_util.oracle_block_starts(big.comp, 64 << 20)
    assert status == 1 and len(blocks) == big.total
    parts = _large(mods, big)
    assert parts >= 0.97 * len(blocks), (parts, len(blocks))
    first = dc.large_stream(False, lead=False)
    _large(mods, first, window=dc.HISTORY, min_parts=int(0.97 * first.total))


@pytest.mark.parametrize("markers", [True, False])
def test_part_mode_sub_starts_inside_crafted_blocks(mods, markers):
    _, inf, zr = mods
    big = dc.large_stream(markers, big=4)
    _large(mods, big, subblock=True, min_parts=big.blocks if markers else int(0.97 * big.total))
    assert inf.inflate_large_last_subparts() > 0, _err(zr)
    # no noise in front: a 32 KiB window, and the first parts' copies reach into it
    first = dc.large_stream(markers, big=4, lead=False)
    _large(mods, first, subblock=True, window=dc.HISTORY, min_parts=first.blocks if markers else int(0.97 * first.total))
    assert inf.inflate_large_last_subparts() > 0, _err(zr)


def test_packed_part_layout(mods):
    torch, inf, zr = mods
    info = (4 * C.c_int32)()
    assert zr.rocm.lib().zng_rocm_device_info(info) == 0
    cus = int(info[0])
    big = dc.large_stream(True, tiny=12 * cus + 200)
    assert big.blocks >= 12 * cus + 200 and set(big.share) == set(dc.kinds())
    plain = _cpython(big.comp)
    dst = torch.zeros(len(plain) + 64, dtype=torch.uint8, device="cuda")
    piece = 4 << 20
    assert len(big.comp) < piece                          # ONE piece holds all the parts: their count is that launch's
    st, n, used, parts, passes, host = inf.inflate_large_pieces_dev(_dev(torch, big.comp), dst, piece_bytes=piece)
    assert passes == 1, passes
    assert (st, n, used, host) == (1, len(plain), len(big.comp), 0), (st, n, used, host, _err(zr))
    assert parts > 12 * cus, (parts, cus, _err(zr))
    assert dst[:n].cpu().numpy().tobytes() == plain and int(dst[n:].max()) == 0


@pytest.mark.parametrize("name", ["dist-over", "no-eob", "dist-unused-code", "16-overrun"])
def test_refusals_deep_in_a_stream_of_parts(mods, name):
    torch, inf, zr = mods
    bad = dc.large_stream(True, bad=name).comp
    assert len(bad) >= (128 << 10)
    ost, omsg, oout, _ = inflate_util.oracle_inflate(bad, cap=8 << 20)
    assert ost == -3 and len(oout) > (128 << 10)
    dst = torch.zeros(len(oout) + 4096, dtype=torch.uint8, device="cuda")
    st, n, used, parts = inf.inflate_large_dev(_dev(torch, bad), dst)
    assert (st, _err(zr)) == (ost, omsg) and n == len(oout) and parts == 0, (st, n, parts, _err(zr), omsg, len(oout))
    assert dst[:n].cpu().numpy().tobytes() == oout
