"""zng_rocm_compress_streams2_dev and zng_rocm_compress_members_dev: many device-resident streams deflated at any level and
strategy and wrapped as raw / zlib / gzip members, in their own buffers or back to back in one file, through the C ABI.
Oracles: CPython's zlib (decompress with wbits -15 / 15 / 31, which also judges every trailer; adler32 / crc32 for the result
words; gzip_files.oracle_table for the file), and for the deflate data the library's own raw engines, whose bytes the new calls
must repeat: zng_rocm_deflate_strategy_streams_dev at levels 1..9, zng_rocm_deflate_strategy_block_dev at level 0.

One batch serves every test: text of data_lcet10.txt in sizes around the block cut (61440), the stored cut (65535) and the
segment cut at small totals (131072), and two jobs of seeded random bytes.  Every plaintext and every output sits at an odd
device address inside 0xAB, and every run checks that no 0xAB outside the members' own bytes has changed."""
import ctypes as C
import importlib
import os
import struct
import zlib

import numpy as np
import pytest

from gzip_files import oracle_table

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, BUF_ERROR = -3, -5
TEXT_SIZES = (0, 1, 5, 61439, 61440, 61441, 65535, 65536, 131071, 131072, 131073, 200000, 2 * 131072 + 17)
RANDOM_SIZES = (65536, 70001)
RANDOM_AT = len(TEXT_SIZES)                       # the job of 65536 random bytes
DICT = 32768
NOT_FINAL, SYNC_FLUSH = 1, 2
# the raw variant of the batch: a 32 KiB dict_len in front of two jobs, and each block flag
RAW_DICT = {2: DICT, 11: DICT}
RAW_FLAGS = {1: NOT_FINAL, 3: NOT_FINAL | SYNC_FLUSH, 4: SYNC_FLUSH, 6: NOT_FINAL | SYNC_FLUSH, 12: NOT_FINAL, 13: NOT_FINAL | SYNC_FLUSH}
COMBOS = [(-1, 0), (0, 0), (1, 0), (6, 0), (9, 0), (6, 1), (6, 2), (6, 3), (6, 4)]      # (level, strategy)
WBITS = (-15, 15, 31)


@pytest.fixture(scope="module")
def mods():
    import torch
    zr = importlib.import_module("zlib-ng_amd")
    zr.init(0)
    return torch, importlib.import_module("zlib-ng_amd.deflate"), importlib.import_module("zlib-ng_amd.inflate"), zr


class Batch:
    """the plaintexts in one device arena of 0xAB: job i at an address that is ODDS[i % 8] modulo 16, DICT bytes of text directly
    in front of the jobs of RAW_DICT"""
    ODDS = (5, 1, 15, 8, 3, 0, 11, 6)

    def __init__(self, torch):
        with open(os.path.join(ROOT, "tests", "golden", "ref_fixtures", "data_lcet10.txt"), "rb") as f:
            lcet = f.read()
        rng = np.random.default_rng(0x5EED)
        self.plain, self.hist, self.off = [], [], []
        arena, at = bytearray(), 0
        for i, n in enumerate(TEXT_SIZES + RANDOM_SIZES):
            start = (i * 29989) % (len(lcet) - n - DICT)
            hist = lcet[start:start + DICT] if i in RAW_DICT else b""
            data = lcet[start + DICT:start + DICT + n] if i < len(TEXT_SIZES) else rng.bytes(n)
            gap = 16 + (self.ODDS[i % 8] - (at + 16 + len(hist))) % 16
            arena += b"\xab" * gap + hist + data
            at += gap + len(hist)
            assert at % 16 == self.ODDS[i % 8]
            self.off.append(at)
            at += n
            self.plain.append(data)
            self.hist.append(hist)
        arena += b"\xab" * 64
        self.n = len(self.plain)
        self.src = torch.from_numpy(np.frombuffer(bytes(arena), dtype=np.uint8).copy()).cuda()
        assert self.src.data_ptr() % 16 == 0
        self.views = [self.src[o:o + len(p)] for o, p in zip(self.off, self.plain)]

    def dict_len(self, raw_variant):
        return [RAW_DICT.get(i, 0) if raw_variant else 0 for i in range(self.n)]

    def flags(self, raw_variant):
        return [RAW_FLAGS.get(i, 0) if raw_variant else 0 for i in range(self.n)]


@pytest.fixture(scope="module")
def batch(mods):
    return Batch(mods[0])


def tail_len(fmt):
    return (0, 4, 8)[fmt]


def want_header(fmt, level, strategy):
    lv = 6 if level == -1 else level
    if fmt == 1:
        c = zlib.compressobj(lv, zlib.DEFLATED, 15, 8, strategy)
        return (c.compress(b"x") + c.flush())[:2]
    if fmt == 2:
        return bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 2 if lv == 9 else 4 if (strategy >= 2 or lv < 2) else 0, 3])
    return b""


def check_value(fmt, plain):
    return zlib.crc32(plain) if fmt == 2 else zlib.adler32(plain)


class Streams2:
    """one zng_rocm_compress_streams2_dev call over the batch (or the jobs `only`): member i in a buffer of exactly the bound at
    an odd address inside an arena of 0xAB"""

    def __init__(self, mods, batch, fmt, level, strategy=0, raw_variant=False, round_bytes=0, stream=None, only=None, mutate=None,
                 call_fmt=None, results=True):
        torch, dfl, _, zr = mods
        self.fmt, self.batch = fmt, batch
        self.idx = list(range(batch.n)) if only is None else list(only)
        caps = [dfl.compress_streams2_bound(len(batch.plain[i]), fmt) for i in self.idx]
        self.out_off, at = [], 0
        for k, cap in enumerate(caps):
            at += 16 + (Batch.ODDS[(k + 3) % 8] - (at + 16)) % 16
            self.out_off.append(at)
            at += cap
        self.arena = torch.full((at + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        assert self.arena.data_ptr() % 16 == 0
        self.results = torch.full((len(self.idx), 2), -0x54545455, dtype=torch.int32, device="cuda")       # 0xABABABAB
        dl, fl = batch.dict_len(raw_variant), batch.flags(raw_variant)
        self.jobs = dfl.stream_jobs([batch.views[i] for i in self.idx], [self.arena[o:o + c] for o, c in zip(self.out_off, caps)],
                                    [dl[i] for i in self.idx], [fl[i] for i in self.idx])
        if mutate:
            mutate(self.jobs)
        torch.cuda.synchronize()
        self.status = dfl.compress_streams2_dev(self.jobs, len(self.idx), self.results if results else None,
                                                fmt if call_fmt is None else call_fmt, level, strategy, round_bytes, stream)
        self.rounds = dfl.compress_streams2_last_rounds()
        self.error = zr.rocm.lib().zng_rocm_last_error().decode()
        if stream is not None:
            stream.synchronize()
        else:
            torch.cuda.synchronize()
        self.res = [(int(a) & 0xffffffff, int(b) & 0xffffffff) for a, b in self.results.cpu().tolist()]
        host = self.arena.cpu().numpy()
        self.untouched = bool((host == 0xAB).all()) and all(r == (0xABABABAB, 0xABABABAB) for r in self.res)
        self.outs = []
        if self.status == 0:
            for o, (n, _), cap in zip(self.out_off, self.res, caps):
                assert n <= cap, (n, cap)
                self.outs.append(host[o:o + n].tobytes())
                host[o:o + n] = 0xAB
            assert (host == 0xAB).all(), "a byte outside the members' own bytes was written"


class Members:
    """one zng_rocm_compress_members_dev call over the batch: the file at an odd address inside 0xAB; cap = dst_cap"""

    def __init__(self, mods, batch, fmt, level, cap, strategy=0, raw_variant=False, round_bytes=0, checks=True, odd=7, mutate=None):
        torch, dfl, _, zr = mods
        self.cap = cap
        self.whole = torch.full((16 + cap + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        self.dst = self.whole[odd:odd + cap] if cap else None
        self.offsets = torch.full((batch.n + 1,), -0x5454545454545455, dtype=torch.int64, device="cuda")
        self.checks = torch.full((batch.n,), -0x54545455, dtype=torch.int32, device="cuda") if checks else None
        self.jobs = dfl.stream_jobs(batch.views, None, batch.dict_len(raw_variant), batch.flags(raw_variant))
        if mutate:
            mutate(self.jobs)
        torch.cuda.synchronize()
        self.status = dfl.compress_members_dev(self.jobs, batch.n, self.dst, self.offsets, fmt, level, strategy, round_bytes, self.checks)
        self.rounds = dfl.compress_streams2_last_rounds()
        torch.cuda.synchronize()
        self.off = [int(v) for v in self.offsets.cpu().tolist()]
        self.chk = [int(v) & 0xffffffff for v in self.checks.cpu().tolist()] if checks else None
        host = self.whole.cpu().numpy()
        # nothing in front of the file, nothing at or behind d_dst + dst_cap
        assert (host[:odd] == 0xAB).all() and (host[odd + cap:] == 0xAB).all()
        self.untouched = bool((host == 0xAB).all()) and all(v == -0x5454545454545455 for v in self.off)
        self.file = host[odd:odd + min(cap, max(self.off[-1], 0))].tobytes() if self.status == 0 else b""
        self.behind = host[odd + min(cap, max(self.off[-1], 0)):odd + cap]


# ---- the references: computed once, shared ----------------------------------------------------------------------------------
_raw = {}


def raw_reference(mods, batch, level, strategy, raw_variant):
    """the deflate data of every job from the existing engines: [bytes]"""
    torch, dfl, _, _ = mods
    lv = 6 if level == -1 else level
    key = (lv, strategy, raw_variant)
    if key not in _raw:
        dl, fl = batch.dict_len(raw_variant), batch.flags(raw_variant)
        if lv == 0:
            outs = []
            for i in range(batch.n):
                dst, n = dfl.deflate_dev(batch.src, level=0, length=len(batch.plain[i]), offset=batch.off[i], dict_len=dl[i], flags=fl[i],
                                         strategy=strategy)
                outs.append(dst[:n].cpu().numpy().tobytes())
        else:
            b = dfl.StreamsBatch(batch.src, batch.off, [len(p) for p in batch.plain], dl, fl)
            b.run(level=lv, strategy=strategy)
            outs = [b.compressed(i) for i in range(batch.n)]
        _raw[key] = outs
    return _raw[key]


_runs = {}


def streams2(mods, batch, fmt, level, strategy=0):
    """the one-round run of the whole batch (format 0: the raw variant), shared by the tests that compare against it"""
    key = (fmt, level, strategy)
    if key not in _runs:
        _runs[key] = Streams2(mods, batch, fmt, level, strategy, raw_variant=(fmt == 0))
    return _runs[key]


def inflate_job(fmt, member, hist, flags):
    """(plaintext, whether the stream ended, bytes left over) from CPython"""
    d = zlib.decompressobj(WBITS[fmt], zdict=hist) if hist else zlib.decompressobj(WBITS[fmt])
    plain = d.decompress(member)
    return plain, d.eof, d.unused_data


# ---- formats, levels and strategies; parity with the engines ----------------------------------------------------------------
@pytest.mark.parametrize("fmt", [0, 1, 2])
@pytest.mark.parametrize("level, strategy", COMBOS)
def test_formats_levels_and_parity(mods, batch, fmt, level, strategy):
    r = streams2(mods, batch, fmt, level, strategy)
    assert r.status == 0 and r.rounds == 1, (r.status, r.error)
    raw_variant = fmt == 0
    want_raw = raw_reference(mods, batch, level, strategy, raw_variant)
    dl, fl = batch.dict_len(raw_variant), batch.flags(raw_variant)
    head, tail = want_header(fmt, level, strategy), tail_len(fmt)
    for i, member in enumerate(r.outs):
        plain = batch.plain[i]
        assert r.res[i] == (len(member), check_value(fmt, plain)), i
        assert member[:len(head)] == head, i
        if fmt == 1:
            assert member[-4:] == struct.pack(">I", zlib.adler32(plain)), i
        if fmt == 2:
            assert member[-8:] == struct.pack("<II", zlib.crc32(plain), len(plain)), i
        # the bytes between header and trailer are the engine's
        assert member[len(head):len(member) - tail] == want_raw[i], (i, len(member), len(want_raw[i]))
        got, eof, left = inflate_job(fmt, member, batch.hist[i] if dl[i] else b"", fl[i])
        assert got == plain and left == b"" and eof == (not fl[i] & NOT_FINAL), i
        if fmt and not fl[i]:
            assert zlib.decompress(member, WBITS[fmt]) == plain, i
    if (level, strategy) == (0, 0):
        for i, member in enumerate(r.outs):                              # the closed form of the stored size
            n = len(batch.plain[i])
            assert len(member) == len(head) + n + 5 * max(1, -(-n // 65535)) + (5 if fl[i] == 3 else 0) + tail, i
            if fl[i] == (NOT_FINAL | SYNC_FLUSH):                        # the sync marker behind the last block, which is not final
                assert member[:len(member) - tail].endswith(b"\x00\x00\x00\xff\xff") and member[len(head)] == 0, i


def test_random_job_is_smaller_than_through_the_level_1_class(mods, batch):
    torch, dfl, _, _ = mods
    r = streams2(mods, batch, 2, 6)
    plain = batch.plain[RANDOM_AT]
    assert len(plain) == 65536
    src = torch.from_numpy(np.frombuffer(plain, dtype=np.uint8).copy()).cuda()
    w = dfl.WrappedBatch(src, [0], [len(plain)], 2)
    w.run()
    torch.cuda.synchronize()
    old = int(w.results.cpu()[0, 0])
    assert zlib.decompress(w.compressed(0), 31) == plain
    assert len(r.outs[RANDOM_AT]) < old, (len(r.outs[RANDOM_AT]), old)


# ---- the file form ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, level", [(0, 6), (1, 6), (2, 6), (2, 0), (1, 0)])
def test_file_form(mods, batch, fmt, level):
    torch, dfl, inf, _ = mods
    one = streams2(mods, batch, fmt, level)
    want_file = b"".join(one.outs)
    m = Members(mods, batch, fmt, level, cap=len(want_file) + 100, raw_variant=(fmt == 0))
    assert m.status == 0 and m.rounds == 1
    sums = [0]
    for member in one.outs:
        sums.append(sums[-1] + len(member))
    assert m.off == sums                                                 # the running sum
    assert m.file == want_file and (m.behind == 0xAB).all()
    assert m.chk == [check_value(fmt, p) for p in batch.plain]
    if fmt == 2:
        rows, plain, end = oracle_table(m.file)
        assert plain == b"".join(batch.plain) and end == len(m.file) and len(rows) == batch.n
        assert [row[0] for row in rows] == m.off[:-1]
        assert [(row[3], row[4]) for row in rows] == [(len(p), zlib.crc32(p)) for p in batch.plain]
        # ... and the library's own readers: the file through the member reader, the members through the many-stream one
        total = sum(len(p) for p in batch.plain)
        filedev = torch.from_numpy(np.frombuffer(m.file, dtype=np.uint8).copy()).cuda()
        back = torch.zeros(total + 64, dtype=torch.uint8, device="cuda")
        st, out_len, in_used, grows, nmembers, _ = inf.gunzip_members_dev(filedev, back[:total])
        assert (st, out_len, in_used, nmembers) == (1, total, len(m.file), batch.n)
        assert back[:total].cpu().numpy().tobytes() == plain and grows == rows
    elif fmt == 1:
        data, at = m.file, 0
        for i, p in enumerate(batch.plain):
            assert at == m.off[i]
            d = zlib.decompressobj(15)
            assert d.decompress(data[at:]) == p and d.eof, i
            at = len(data) - len(d.unused_data)
        assert at == len(data)
    else:
        dl, fl = batch.dict_len(True), batch.flags(True)
        for i, p in enumerate(batch.plain):
            got, eof, left = inflate_job(0, m.file[m.off[i]:m.off[i + 1]], batch.hist[i] if dl[i] else b"", fl[i])
            assert got == p and left == b"" and eof == (not fl[i] & NOT_FINAL), i


@pytest.mark.parametrize("fmt", [1, 2])
def test_members_back_through_uncompress_streams(mods, batch, fmt):
    torch, _, inf, _ = mods
    one = streams2(mods, batch, fmt, 6)
    lens = [len(p) for p in batch.plain]
    out_off = [sum(lens[:i]) for i in range(batch.n)]
    back = torch.zeros(sum(lens) + 64, dtype=torch.uint8, device="cuda")
    b = inf.InflateDevBatch(one.arena, one.out_off, [n for n, _ in one.res], back, out_off, lens)
    b.run_wrapped(fmt)
    torch.cuda.synchronize()
    assert b.rows() == [(1, n, c, "") for n, (c, _) in zip(lens, one.res)]
    assert back[:sum(lens)].cpu().numpy().tobytes() == b"".join(batch.plain)


# ---- dst_cap ----------------------------------------------------------------------------------------------------------------
def test_dst_cap(mods, batch):
    one = streams2(mods, batch, 2, 6)
    want_file = b"".join(one.outs)
    sums = [0]
    for member in one.outs:
        sums.append(sums[-1] + len(member))
    exact = Members(mods, batch, 2, 6, cap=len(want_file))
    assert exact.status == 0 and exact.off == sums and exact.file == want_file
    # one byte less, a cut inside a member's deflate data, inside a header and inside a trailer, and no room at all
    for cap in (len(want_file) - 1, sums[9] + 4000, sums[5] + 3, sums[12] - 2, 1, 0):
        m = Members(mods, batch, 2, 6, cap=cap, checks=(cap != 1))
        assert m.status == 0 and m.off == sums and m.off[-1] > cap, cap
        assert m.file == want_file[:cap], cap                            # Members itself looks at the bytes at and behind dst_cap
        if m.chk is not None:
            assert m.chk == [zlib.crc32(p) for p in batch.plain]
    # level 0 moves the plaintext itself: the same cut there
    zero = b"".join(streams2(mods, batch, 2, 0).outs)
    m = Members(mods, batch, 2, 0, cap=len(zero) - 70000)
    assert m.status == 0 and m.off[-1] == len(zero) and m.file == zero[:len(zero) - 70000]


# ---- rounds -----------------------------------------------------------------------------------------------------------------
def plan_rounds(lens, round_bytes):
    rounds, first = [], 0
    while first < len(lens):
        last, total = first, 0
        while last < len(lens) and (last == first or total + lens[last] <= round_bytes):
            total += lens[last]
            last += 1
        rounds.append(last - first)
        first = last
    return rounds


@pytest.mark.parametrize("fmt, level", [(2, 6), (0, 6), (1, 0)])
def test_rounds(mods, batch, fmt, level):
    rb = 256 << 10
    lens = [len(p) for p in batch.plain]
    plan = plan_rounds(lens, rb)
    firsts = [sum(plan[:k]) for k in range(len(plan))]
    assert len(plan) > 3 and lens[12] > rb and plan[firsts.index(12)] == 1                  # the over-long job is alone in its round
    one = streams2(mods, batch, fmt, level)
    r = Streams2(mods, batch, fmt, level, raw_variant=(fmt == 0), round_bytes=rb)
    assert r.status == 0 and r.rounds == len(plan)
    assert r.outs == one.outs and r.res == one.res
    want_file = b"".join(one.outs)
    whole = Members(mods, batch, fmt, level, cap=len(want_file), raw_variant=(fmt == 0))
    m = Members(mods, batch, fmt, level, cap=len(want_file), raw_variant=(fmt == 0), round_bytes=rb)
    assert m.status == 0 and m.rounds == len(plan) and whole.rounds == 1
    assert m.file == whole.file == want_file and m.off == whole.off and m.chk == whole.chk
    # one job per round
    tiny = Members(mods, batch, fmt, level, cap=len(want_file), raw_variant=(fmt == 0), round_bytes=1)
    assert tiny.rounds == len(plan_rounds(lens, 1)) and tiny.file == want_file and tiny.off == whole.off


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _set(i, **fields):
    def mutate(jobs):
        for k, v in fields.items():
            setattr(jobs[i], k, v)
    return mutate


def test_refusals_leave_everything_untouched(mods, batch):
    _, dfl, _, _ = mods
    few = [1, 3, 11]
    bound = dfl.compress_streams2_bound(len(batch.plain[3]), 2)
    cases = [
        (EINVAL, dict(call_fmt=3)), (EINVAL, dict(call_fmt=-1)), (EINVAL, dict(level=10)), (EINVAL, dict(level=-2)),
        (EINVAL, dict(strategy=5)), (EINVAL, dict(strategy=-1)), (EINVAL, dict(results=False)),
        (EINVAL, dict(mutate=_set(1, in_ptr=None))), (EINVAL, dict(mutate=_set(1, out_ptr=None))),
        (EINVAL, dict(mutate=_set(2, dict_len=1))), (EINVAL, dict(mutate=_set(2, flags=NOT_FINAL))),
        (EINVAL, dict(mutate=_set(2, flags=SYNC_FLUSH))), (EINVAL, dict(fmt=0, mutate=_set(0, dict_len=32769))),
        (EINVAL, dict(fmt=0, mutate=_set(0, flags=4))), (EINVAL, dict(mutate=_set(1, in_len=0xfffffff0))),
        (BUF_ERROR, dict(mutate=_set(1, out_cap=bound - 1))),
    ]
    for want, kw in cases:
        args = dict(fmt=2, level=6, strategy=0)
        args.update(kw)
        r = Streams2(mods, batch, args.pop("fmt"), args.pop("level"), args.pop("strategy"), only=few, **args)
        assert r.status == want and r.untouched and r.rounds == 0, (kw, r.status, r.error)
    for want, fmt, kw in [(EINVAL, 3, {}), (EINVAL, 2, dict(strategy=7)), (EINVAL, 2, dict(mutate=_set(4, dict_len=5))),
                          (EINVAL, 1, dict(mutate=_set(4, flags=3))), (EINVAL, 0, dict(mutate=_set(4, flags=8))),
                          (EINVAL, 2, dict(mutate=_set(4, in_ptr=None)))]:
        m = Members(mods, batch, fmt, 6, cap=4096, **kw)
        assert m.status == want and m.untouched and m.rounds == 0, (fmt, kw)
    # the pointers of the call itself
    lib = mods[3].rocm.lib()
    m = Members(mods, batch, 2, 6, cap=4096, mutate=_set(0, dict_len=1))         # (a destination to look at)
    assert lib.zng_rocm_compress_members_dev(2, 6, 0, C.byref(m.jobs), batch.n, None, 4096, 0, m.offsets.data_ptr(), None, None) == EINVAL
    assert lib.zng_rocm_compress_members_dev(2, 6, 0, C.byref(m.jobs), batch.n, m.whole.data_ptr(), 4096, 0, None, None, None) == EINVAL
    assert lib.zng_rocm_compress_members_dev(2, 6, 0, None, batch.n, m.whole.data_ptr(), 4096, 0, m.offsets.data_ptr(), None, None) == EINVAL
    mods[0].cuda.synchronize()
    assert int(m.whole.min()) == 0xAB and int(m.offsets.max()) == -0x5454545454545455
    # no jobs: no work, and nothing is asked of the pointers
    assert lib.zng_rocm_compress_streams2_dev(2, 6, 0, None, 0, 0, None, None) == 0
    assert lib.zng_rocm_compress_members_dev(2, 6, 0, None, 0, None, 0, 0, None, None, None) == 0


# ---- the stream -------------------------------------------------------------------------------------------------------------
def test_on_a_stream_of_its_own(mods, batch):
    torch = mods[0]
    one = streams2(mods, batch, 2, 6)
    st = torch.cuda.Stream()
    r = Streams2(mods, batch, 2, 6, stream=st)                           # synchronises that stream only, then reads
    assert r.status == 0 and r.outs == one.outs and r.res == one.res
    mods[3].rocm.lib().zng_rocm_stream_release(C.c_void_p(st.cuda_stream))
