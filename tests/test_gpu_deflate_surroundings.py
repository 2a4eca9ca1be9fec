"""GPU: every device deflate engine at all 16 input phases, amid bytes built to be mistaken for input (tests/surround_cases.py).

include/zng_rocm.h gives every deflate call an input at any alignment with dict_len bytes of history in front of it, and says
nothing of the bytes behind the input or in front of the history: the output is a function of the input alone.
One test per engine; each makes one call (or one small set of calls) over the engine's case list laid out three times in one
device tensor -- "zeros", "bait", "noise" -- and asserts for every job, in this order:

  a  an independent reader: zlib.decompressobj(-15, zdict=H) restores exactly P with eof set and nothing unused (zlib.decompress
     / gzip.decompress for the wrapped formats, whose trailers check P's Adler-32 / CRC-32); deflate_parse finds no distance
     above 32506 (the window forms: their cap) and none that reaches in front of the first byte of H;
  b  the check word the call returns equals zlib.adler32(P) / zlib.crc32(P);
  c  the bytes written for one (H, P) are the same in every layout and at every input and output phase.  "zeros" at phase 0 is
     what every older test runs, so this ties every other configuration to it; a and b do not involve the device's own output;
  d  the destination was filled with 0xA5: nothing outside [out, out + out_cap) has changed (64 guard bytes on both sides of
     every slot), and the source tensor is bit-identical after the call.

a is computed once per distinct output of a case: a stray read shows as other bytes, which are then read on their own.
Output phase: the calls that ask no alignment of `out` (the rows engine, its strategy / window / dictionary forms and
compress_streams2) get every out % 16; the level-1 class calls demand 4-byte alignment, get the four multiples of 4 and must
refuse anything else with ZNG_ROCM_EINVAL and write nothing."""
import ctypes as C
import gzip
import importlib
import zlib

import numpy as np
import pytest

import deflate_parse as dp
import matcher_cases as mc
import surround_cases as sc
from gpu_common import product, torch_mod

pytestmark = pytest.mark.gpu

GUARD, FILL, EINVAL = 64, 0xA5, -3
FLUSH = 3                                   # ZNG_ROCM_BLOCK_NOT_FINAL | ZNG_ROCM_BLOCK_SYNC_FLUSH
END = b"\x03\x00"                           # a final empty static block: what ends a stream whose last job was not final


@pytest.fixture(scope="module")
def mods():
    zr = product()
    zr.init()
    return zr, importlib.import_module("zlib-ng_amd.deflate")


_IMAGES = {}


def _image(name, history=True):
    """(Image, device tensor) of a list, made once and never changed (every test checks that it has not)"""
    if (name, history) not in _IMAGES:
        im = sc.build_image(sc.placements(name), history=history)
        src = torch_mod().from_numpy(im.host).cuda()
        assert src.data_ptr() % 16 == 0
        _IMAGES[name, history] = (im, src)
    return _IMAGES[name, history]


def _flags(j):
    """NOT_FINAL | SYNC_FLUSH on a quarter of the cases: by the case, so that every placement of it has the same"""
    return FLUSH if j.key % 4 == 1 else 0


class Slots:
    """The destination of one call: job i's slot of caps[i] bytes with at least GUARD bytes on both sides, everything 0xA5.
    align 1: out % 16 takes every value; 4: the four multiples of 4."""

    def __init__(self, caps, align):
        torch = torch_mod()
        self.caps, self.off, pos = [int(c) for c in caps], [], 4096
        for i, cap in enumerate(self.caps):
            o = pos + GUARD
            o += (((5 * i + i // 16) % 16 if align == 1 else 4 * ((i + i // 4) % 4)) - o) % 16
            self.off.append(o)
            pos = o + cap
        self.dst = torch.full((pos + GUARD + 4096,), FILL, dtype=torch.uint8, device="cuda")
        assert self.dst.data_ptr() % 16 == 0
        assert len(self.caps) < 16 or {o % 16 for o in self.off} == set(range(0, 16, align))

    def point(self, jobs):
        for i, o in enumerate(self.off):
            jobs[i].out_ptr = self.dst.data_ptr() + o
            jobs[i].out_cap = self.caps[i]

    def members(self, lens):
        torch_mod().cuda.synchronize()
        self.host = self.dst.cpu().numpy()
        assert all(int(n) <= cap for n, cap in zip(lens, self.caps))
        return [self.host[o:o + int(n)].tobytes() for o, n in zip(self.off, lens)]

    def assert_contained(self):
        outside = np.ones(self.host.size, dtype=bool)
        for o, cap in zip(self.off, self.caps):
            outside[o:o + cap] = False
        assert bool((self.host[outside] == FILL).all()), "bytes outside [out, out + out_cap) were written"


def _reslot(batch, align):
    """the batch classes of zlib-ng_amd.deflate lay their slots back to back: the same jobs, guarded slots at swept phases"""
    slots = Slots(batch.bounds, align)
    slots.point(batch.jobs)
    batch.dst, batch.out_off = slots.dst, slots.off
    return slots


def _jobs(dfl, im, src, with_history=True, flags=True):
    jobs = (dfl.StreamJob * len(im.jobs))()
    for i, j in enumerate(im.jobs):
        jobs[i].in_ptr = src.data_ptr() + j.in_off
        jobs[i].in_len = j.case.n
        jobs[i].dict_len = len(j.case.H) if with_history else 0
        jobs[i].flags = _flags(j) if flags else 0
    return jobs


RAW_AT = {"raw": (0, 0), "zlib12": (2, 4), "gzip12": (12, 8), "zlib": (2, 4), "gzip": (10, 8), "zdict": (6, 4)}


def _read(c, H, member, fmt, final, cap, wbits):
    """assertion a for one output of one case"""
    if fmt in ("zlib12", "zlib"):
        assert zlib.decompress(member) == c.P, c
    elif fmt in ("gzip12", "gzip"):
        assert gzip.decompress(member) == c.P, c
    elif fmt == "zdict":
        d = zlib.decompressobj(zdict=H)
        assert d.decompress(member) == c.P and d.eof and d.unused_data == b"", c
    head, trail = RAW_AT[fmt]
    raw = member[head:len(member) - trail] + (b"" if final else END)
    d = zlib.decompressobj(-wbits, zdict=H) if H else zlib.decompressobj(-wbits)
    assert d.decompress(raw) == c.P, c
    assert d.eof and d.unused_data == b"", c
    parsed = dp.parse(raw, history=H)
    assert parsed.data == c.P, c
    cov = mc.coverage(parsed, 0, c.n, len(H))
    assert cov.max_dist <= cap, (c, cov.max_dist)
    assert cov.min_reach >= 0, (c, cov.min_reach)
    return parsed, cov


def _verify(im, members, fmt="raw", shared=b"", checks=None, check_fn=zlib.adler32, cap=sc.MAX_DIST, wbits=15, flags=True,
            extra=None):
    """a, b for every job, then c over all of them.  shared: the dictionary object's bytes (no job has history of its own).
    extra(case, parsed, cover): what the engine promises on top."""
    assert len(members) == len(im.jobs)
    read = {}
    for i, (j, m) in enumerate(zip(im.jobs, members)):
        c = j.case
        if (j.key, m) not in read:
            H = (shared or c.H)[-32768:]
            parsed, cov = _read(c, H, m, fmt, not (flags and _flags(j)), cap, wbits)
            if extra:
                extra(c, parsed, cov)
            read[j.key, m] = True
        if checks is not None:
            assert int(checks[i]) == check_fn(c.P), (c, j.layout, j.phase)
    first = {}
    for j, m in zip(im.jobs, members):
        k = first.setdefault(j.key, (j, m))
        assert m == k[1], "%s: %s at phase %d differs from %s at phase %d" % (j.case, j.layout, j.phase, k[0].layout, k[0].phase)
    assert {j.layout for j in im.jobs} == set(sc.LAYOUTS)


def _assert_source_untouched(im, src):
    assert np.array_equal(src.cpu().numpy(), im.host), "the source tensor changed"


def _refuses_misaligned_out(call, jobs, n, slots, results):
    """a call that demands 4-byte alignment: job 1's out moved by 1, 2, 3 -> ZNG_ROCM_EINVAL, nothing written"""
    torch = torch_mod()
    keep = jobs[1].out_ptr
    for shift in (1, 2, 3):
        jobs[1].out_ptr = keep + shift
        slots.dst.fill_(FILL)
        results.zero_()
        assert call(jobs, n, results) == EINVAL, shift
        torch.cuda.synchronize()
        assert bool((slots.dst == FILL).all()) and not bool(results.any()), shift
    jobs[1].out_ptr = keep


def test_level_1_class_quick_kernel(mods):
    """deflate_quick_kernel through zng_rocm_deflate_quick_dev: flags 0 and NOT_FINAL | SYNC_FLUSH, history of 0 .. 32768 bytes"""
    zr, dfl = mods
    im, src = _image("main")
    b = dfl.QuickBatch(src, [j.in_off for j in im.jobs], [j.case.n for j in im.jobs], [len(j.case.H) for j in im.jobs],
                       [_flags(j) for j in im.jobs])
    slots = _reslot(b, 4)
    b.run()
    res = b.results.cpu().numpy().astype(np.int64) & 0xffffffff
    _verify(im, slots.members(res[:, 0]), checks=res[:, 1])
    slots.assert_contained()
    _assert_source_untouched(im, src)
    lib = zr.rocm.lib()
    _refuses_misaligned_out(lambda jobs, n, r: lib.zng_rocm_deflate_quick_dev(C.byref(jobs), n, zr.rocm._dev_ptr(r), zr.rocm._stream_ptr(None)),
                            b.jobs, 8, slots, b.results)


@pytest.mark.parametrize("fmt", (0, 1))
def test_level_1_class_dictionary_kernel(mods, fmt):
    """deflate_quick_dict_kernel through WrappedBatch.run_dict: the dictionary object is H, the front bait stands directly in
    front of `in` -- where the history of a job of its own would stand"""
    zr, dfl = mods
    im, src = _image("dict", history=False)
    H = bytes(sc.body(sc.FRONT_COPY, np.random.default_rng(0x4443)))
    dic = dfl.Dictionary(H)
    try:
        b = dfl.WrappedBatch(src, [j.in_off for j in im.jobs], [j.case.n for j in im.jobs], fmt, for_dict=True)
        slots = _reslot(b, 4)
        b.run_dict(dic)
        res = b.results.cpu().numpy().astype(np.int64) & 0xffffffff
        _verify(im, slots.members(res[:, 0]), fmt="zdict" if fmt else "raw", shared=H, checks=res[:, 1], flags=False)
        slots.assert_contained()
        _assert_source_untouched(im, src)
        lib = zr.rocm.lib()
        _refuses_misaligned_out(lambda jobs, n, r: lib.zng_rocm_compress_streams_dict_dev(fmt, dic.h, C.byref(jobs), n, zr.rocm._dev_ptr(r),
                                                                                           zr.rocm._stream_ptr(None)),
                                b.jobs, 8, slots, b.results)
    finally:
        dic.close()


def _streams(mods, name, extra=None, cap=sc.MAX_DIST, **run):
    zr, dfl = mods
    im, src = _image(name)
    b = dfl.StreamsBatch(src, [j.in_off for j in im.jobs], [j.case.n for j in im.jobs], [len(j.case.H) for j in im.jobs],
                         [_flags(j) for j in im.jobs])
    slots = _reslot(b, 1)
    lens = b.run(**run)
    _verify(im, slots.members(lens), cap=cap, wbits=run.get("window_bits", 15), extra=extra)
    slots.assert_contained()
    _assert_source_untouched(im, src)


@pytest.mark.parametrize("level", (1, 6, 9))
def test_rows_engine(mods, level):
    """lz_rows_kernel, emit_dynamic_kernel, the scan and the gather through StreamsBatch.run"""
    _streams(mods, "main", level=level)


@pytest.mark.parametrize("strategy", (3, 2))
def test_rle_front_end(mods, strategy):
    """rle_rows_kernel<false> (Z_RLE: distance 1 alone) and <true> (Z_HUFFMAN_ONLY: no match at all)"""
    assert sum(j.case.D == 1 and not j.case.tiny for j in _image("main")[0].jobs) >= 100

    def extra(c, parsed, cov):
        assert cov.dists <= ({1} if strategy == 3 else set()), (c, cov.dists)
        if strategy == 3 and not c.tiny and c.D == 1:
            assert 1 in mc.coverage(parsed, c.n - c.k, c.n, 0).dists, c          # the run P ends in is a match
    _streams(mods, "main", extra=extra, level=6, strategy=strategy)


def test_static_blocks_emitter(mods):
    """emit_dynamic_kernel<FORCE_STATIC> (Z_FIXED): stored and static blocks alone"""
    def extra(c, parsed, cov):
        assert all(b.btype in (dp.STORED, dp.STATIC) for b in parsed.blocks), c
    _streams(mods, "main", extra=extra, level=6, strategy=4)


@pytest.mark.parametrize("window_bits", (9, 12))
def test_window_form(mods, window_bits):
    """lz_rows_win_kernel: distances inside the cap, read by a reader with that window; a repeat just above the cap, of bytes
    that occur nowhere else, comes out as literals"""
    cap = sc.WINDOW_CAP[window_bits]
    above = []

    def extra(c, parsed, cov):
        if c.unique:
            assert c.D > cap and mc.coverage(parsed, c.n - c.k, c.n, len(c.H)).lits == c.k, c
            above.append(c.D)
    _streams(mods, "win%d" % window_bits, extra=extra, cap=cap, level=6, window_bits=window_bits)
    assert cap + 1 in above


def test_one_stream_call(mods):
    """zng_rocm_deflate_block_dev at level 6 on 300 KiB + 5 (three segments), phases 0, 1, 7, 15, without history and with 300
    bytes of it; its d_out takes any alignment"""
    zr, dfl = mods
    im, src = _image("one")
    lib = zr.rocm.lib()
    slots = Slots([dfl.deflate_bound(j.case.n) for j in im.jobs], 1)
    lens = []
    for i, j in enumerate(im.jobs):
        out_len = C.c_size_t(0)
        rc = lib.zng_rocm_deflate_block_dev(6, zr.rocm._dev_ptr(src, j.in_off), j.case.n, len(j.case.H), 0,
                                            zr.rocm._dev_ptr(slots.dst, slots.off[i]), slots.caps[i], C.byref(out_len),
                                            zr.rocm._stream_ptr(None))
        assert rc == 0, (j.case, rc)
        lens.append(out_len.value)
    _verify(im, slots.members(lens), flags=False)
    slots.assert_contained()
    _assert_source_untouched(im, src)


@pytest.mark.parametrize("fmt", (0, 1))
def test_rows_dictionary_form(mods, fmt):
    """lz_rows_dict_kernel through zng_rocm_compress_streams2_dict_dev at level 6"""
    zr, dfl = mods
    torch = torch_mod()
    im, src = _image("dict", history=False)
    H = bytes(sc.body(sc.FRONT_COPY, np.random.default_rng(0x4443)))
    dic = dfl.Dictionary(H)
    try:
        jobs = _jobs(dfl, im, src, with_history=False, flags=False)
        slots = Slots([dfl.compress_streams2_dict_bound(j.case.n, fmt) for j in im.jobs], 1)
        slots.point(jobs)
        results = torch.zeros((len(im.jobs), 2), dtype=torch.int32, device="cuda")
        assert dfl.compress_streams2_dict_dev(dic, jobs, len(im.jobs), results, fmt, level=6) == 0
        res = results.cpu().numpy().astype(np.int64) & 0xffffffff
        _verify(im, slots.members(res[:, 0]), fmt="zdict" if fmt else "raw", shared=H, checks=res[:, 1], flags=False)
        slots.assert_contained()
        _assert_source_untouched(im, src)
    finally:
        dic.close()


def test_stored_kernel(mods):
    """stored_kernel through zng_rocm_deflate_block_dev at level 0, one call per job: lengths around 65535 and 131070 on top of
    the others; its d_out takes any alignment (every block's payload starts at an odd offset anyway)"""
    zr, dfl = mods
    im, src = _image("stored")
    lib = zr.rocm.lib()
    slots = Slots([dfl.deflate_bound(j.case.n) for j in im.jobs], 1)
    lens = []
    for i, j in enumerate(im.jobs):
        out_len = C.c_size_t(0)
        rc = lib.zng_rocm_deflate_block_dev(0, zr.rocm._dev_ptr(src, j.in_off), j.case.n, len(j.case.H), _flags(j),
                                            zr.rocm._dev_ptr(slots.dst, slots.off[i]), slots.caps[i], C.byref(out_len),
                                            zr.rocm._stream_ptr(None))
        assert rc == 0, (j.case, rc)
        lens.append(out_len.value)

    def extra(c, parsed, cov):
        assert all(b.btype == dp.STORED for b in parsed.blocks[:-1]) and cov.lits == c.n, c
    _verify(im, slots.members(lens), extra=extra)
    slots.assert_contained()
    _assert_source_untouched(im, src)


@pytest.mark.parametrize("call,fmt", (("streams", 1), ("streams", 2), ("streams2", 1), ("streams2", 2)))
def test_wrappers_and_their_checksum_passes(mods, call, fmt):
    """zng_rocm_compress_streams_dev (level-1 class, 12-byte wrappers, out 4-byte aligned) and zng_rocm_compress_streams2_dev
    (level 6, canonical wrappers, no alignment asked): Adler-32 for zlib, CRC-32 for gzip, over plaintexts at every phase"""
    zr, dfl = mods
    torch = torch_mod()
    im, src = _image("dict", history=False)
    n = len(im.jobs)
    check_fn = zlib.adler32 if fmt == 1 else zlib.crc32
    if call == "streams":
        b = dfl.WrappedBatch(src, [j.in_off for j in im.jobs], [j.case.n for j in im.jobs], fmt)
        slots = _reslot(b, 4)
        b.run()
        results, kind = b.results, ("zlib12", "gzip12")[fmt - 1]
    else:
        jobs = _jobs(dfl, im, src, with_history=False, flags=False)
        slots = Slots([dfl.compress_streams2_bound(j.case.n, fmt) for j in im.jobs], 1)
        slots.point(jobs)
        results, kind = torch.zeros((n, 2), dtype=torch.int32, device="cuda"), ("zlib", "gzip")[fmt - 1]
        assert dfl.compress_streams2_dev(jobs, n, results, fmt, level=6) == 0
    res = results.cpu().numpy().astype(np.int64) & 0xffffffff
    _verify(im, slots.members(res[:, 0]), fmt=kind, checks=res[:, 1], check_fn=check_fn, flags=False)
    slots.assert_contained()
    _assert_source_untouched(im, src)
    if call == "streams":
        lib = zr.rocm.lib()
        _refuses_misaligned_out(lambda jobs, k, r: lib.zng_rocm_compress_streams_dev(fmt, C.byref(jobs), k, zr.rocm._dev_ptr(r),
                                                                                     zr.rocm._stream_ptr(None)),
                                b.jobs, 8, slots, b.results)
